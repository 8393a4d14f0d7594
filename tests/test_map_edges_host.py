"""The path-directed map and pre-filter inputs (map_edge_data.py) on the CPU: the oracle's LocalMap and pcl::VoxelGrid equal the plain
restatements on every small family -- insert counts, the point set of every cube, the filtered clouds -- and every family has the
property that makes it worth running on the device (printed, then asserted): a family that was thinned out fails here.  Every
comparison is exact."""
import numpy as np
import pytest

import map_edge_data as med


def _oracle_map(oracle, fam):
    om = oracle.OracleMap(plane_res=fam.create_res or fam.plane_res, line_res=(fam.create_res or fam.plane_res) / 2)
    if fam.window_t is not None:
        om.set_origin(np.array(fam.window_t)); om.shift(np.array(fam.window_t))
    if fam.create_res:
        om.add_surf(fam.warmup)
        om.set_resolution(fam.plane_res / 2, fam.plane_res)
    return om


def _oracle_cubes(om):
    """{linear cube index: points} out of the oracle's export (ascending cube index) and its cube sizes"""
    exp, out, at = om.export(), {}, 0
    for ci in range(med.W * med.H * med.D):
        n = om.L.orc_map_cube_size(om.h, ci)
        if n:
            out[ci] = exp[at:at + n]; at += n
    assert at == len(exp)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(med.SMALL_FAMILIES))
def test_oracle_map_equals_the_plain_restatement(oracle, name):
    fam = med.family(name)
    om = _oracle_map(oracle, fam)
    pm = med.PlainMap(fam.create_res or fam.plane_res)
    if fam.window_t is not None:
        pm.set_origin(fam.window_t); pm.shift(fam.window_t)
    if fam.create_res:
        assert pm.add(fam.warmup) == len(fam.warmup) and pm.size() == om.size() > 1000
        pm.plane_res = fam.plane_res
    assert tuple(om.origin()) == pm.origin == fam.origin()
    for step, cloud in enumerate(fam.clouds):
        assert om.add_surf(cloud) == pm.add(cloud), (name, step)
        assert om.size() == pm.size(), (name, step)
        oc = _oracle_cubes(om)
        assert sorted(oc) == sorted(med.cube_linear(c) for c in pm.cubes), (name, step)
        for c, pts in pm.cubes.items():
            assert np.array_equal(_bits(oc[med.cube_linear(c)]), _bits(pts)), (name, step, c)
    assert np.isfinite(om.export()).all()
    # the probes: five neighbours wherever a cube is found, no two candidates of the first six at one distance -- the order in which an
    # implementation holds a cube's points then does not show in its lists
    found, nbr, d2, idx, cube = om.knn(fam.probes, 6, use_grid=0)
    f = found.astype(bool)
    assert f.sum() >= 0.5 * len(f), (name, int(f.sum()), len(f))
    assert (d2[f][:, 5] < 1e30).all(), f"{name}: a probed cube holds fewer than six points"
    assert (np.diff(d2[f], axis=1) > 0).all(), f"{name}: a probe with two neighbours at one distance"
    for a, b in zip(om.knn(fam.probes, 5, use_grid=1)[:3], om.knn(fam.probes, 5, use_grid=0)[:3]):
        assert np.array_equal(_bits(a[f]) if a.dtype == np.float32 else a, _bits(b[f]) if b.dtype == np.float32 else b), (name, "grid search against brute force")
    for q, fo, c in zip(fam.probes, f, cube):
        want = med.cube_of_point(q, fam.origin())
        assert (not fo and (want is None or med.cube_linear(want) not in oc)) or (fo and med.cube_linear(want) == c), (name, q)
    print(f"{name}: {sum(len(c) for c in fam.clouds)} points in {len(fam.clouds)} inserts, {om.size()} in the map in {len(oc)} cubes, "
          f"{len(f)} probes, {int(f.sum())} with a cube")


@pytest.mark.parametrize("plane_res", [0.2, 0.4])
def test_cube_faces_put_points_on_both_sides_of_every_face(plane_res):
    fam = med.family(f"cube_faces_{plane_res}")
    pts = fam.info["points"]
    seen = set()
    for axis, face, j, at in fam.info["sites"]:
        c = med.cube_coord(pts[at, axis])
        k = round((face + 25.0) / 50.0)  # the cube that begins at this face
        seen.add((axis, face, c - k))
        if j in (0, 1, 3):  # the face itself, one ulp above, 1e-4 above
            # (face + 25 == -50 m with m > 0: the reference truncates and then decrements, the face itself belongs to the cube BELOW)
            want = k - 1 if (j == 0 and face + 25.0 < 0) else k
            assert c == want, (axis, face, j, c)
        else:
            assert c == k - 1, (axis, face, j, c)
    for axis in range(3):
        for face in (med.CUBE_FACES if axis < 2 else med.Z_FACES):
            assert {(axis, face, 0), (axis, face, -1)} <= seen, f"face {face} of axis {axis} has points on one side only"
    assert med.cube_coord(-75.0) == -2 and med.cube_coord(-125.0) == -3 and med.cube_coord(-25.0) == 0 and med.cube_coord(25.0) == 1
    on_face = sum(int(((pts[:, a].astype(np.float64) + 25.0) % 50.0 == 0).sum()) for a in range(3))
    print(f"cube_faces_{plane_res}: {len(pts)} site points, {on_face} coordinates exactly on a face")
    assert on_face >= 2 * (2 * len(med.CUBE_FACES) + len(med.Z_FACES)) + 20
    # the corner (-75, -75, -25) and the 26 points one ulp around it lie in eight cubes
    corner = np.array([-75.0, -75.0, -25.0], np.float32)
    near = pts[(np.abs(pts - corner) < 1e-3).all(1)]
    assert len(near) == 27 and len({med.cube_of_point(p) for p in near}) == 8
    assert med.cube_of_point(corner) == (10 - 2, 10 - 2, 5)


@pytest.mark.parametrize("name", ["window_edge", "window_edge_shifted"])
def test_window_edge_has_an_accepted_and_a_rejected_neighbour_at_every_limit(oracle, name):
    fam = med.family(name)
    pts, origin = fam.info["points"], fam.origin()
    assert len(fam.info["limits"]) == 6
    for axis, lim, a, b in fam.info["limits"]:
        inside = [med.cube_of_point(p, origin) is not None for p in pts[a:b]]
        vals = pts[a:b, axis].astype(np.float64)
        assert vals[0] == lim and any(inside[1:3]) and not all(inside[1:3]), (axis, lim, "the two float neighbours of the limit lie on either side")
        assert inside[5] and sum(inside) >= 2 and sum(inside) <= 4, (axis, lim, inside)
        outermost = med.cube_of_point(pts[a + 5], origin)[axis]
        assert outermost in (0, med.DIMS[axis] - 1)
    if name == "window_edge":
        x = lambda v: med.cube_of_point((v, 0.0, 0.0))
        assert x(-525.0) is None and x(525.0) is None and x(float(med.up(-525.0))) is not None and x(float(med.down(525.0))) is not None
        z = lambda v: med.cube_of_point((0.0, 0.0, v))
        assert z(-275.0) is None and z(275.0) is None and z(float(med.up(-275.0))) is not None and z(float(med.down(275.0))) is not None
    else:
        assert origin == (0, 5, 3) and med.window_limits(origin)[0] == (-25.0, 1025.0)
        assert med.cube_of_point((-25.0, -80.0, 3.0), origin) is not None, "a low limit at c + 25 == 0 is inside: nothing is decremented"
    om = _oracle_map(oracle, fam)
    want = sum(med.cube_of_point(p, origin) is not None for p in fam.clouds[0])
    assert om.add_surf(fam.clouds[0]) == want and 0 < want < len(fam.clouds[0])


@pytest.mark.parametrize("leaf", med.LEAF_RESOLUTIONS)
def test_leaf_faces_straddle_their_faces(leaf):
    triples = med.leaf_triples(leaf)
    assert len(triples) >= 3 * 36
    split = 0
    for axis, L, vals in triples:
        l = med.leaf_index(np.array(vals, np.float32), leaf)
        assert l[0] <= l[1] <= l[2] and l[2] - l[0] <= 1
        split += int(l[0] != l[1] or l[2] != l[1])
    print(f"leaf_faces_{leaf}: {len(triples)} triples, {split} with a neighbour in another leaf than the centre value")
    assert split >= len(triples) / 3, (leaf, split, len(triples))
    fam = med.family(f"leaf_faces_{leaf}")
    sizes = med.leaf_sizes(fam.info["points"], leaf)
    assert sizes.min() >= 1 and sizes.max() <= 4 and (sizes >= 2).sum() >= 0.9 * len(sizes)
    assert (fam.create_res is not None) == (leaf in med.SET_ON_LIVE_MAP)


@pytest.mark.parametrize("name", [n for n in med.SMALL_FAMILIES if n.startswith("rounds")])
def test_rounds_touch_the_number_of_cubes_they_name(name):
    fam = med.family(name)
    for cloud in fam.clouds:
        cubes = {med.cube_of_point(p) for p in cloud}
        assert None not in cubes and len(cubes) == fam.info["n_cubes"]
        assert len(cloud) == 300 * fam.info["n_cubes"]


def test_non_finite_rows_are_where_a_wavefront_would_notice():
    fam = med.family("non_finite")
    for cloud, bad in zip(fam.clouds, fam.info["bad_rows"]):
        nf = ~np.isfinite(cloud).all(1)
        assert np.array_equal(nf, bad) and 230 <= nf.sum() <= 260
        assert nf[0] and nf[-1] and nf[64 * 7] and nf[64 * 7 + 63] and nf[64 * 100:64 * 101].all() and not nf[64 * 99:64 * 100].all()
        for a in range(3):
            assert np.isnan(cloud[:, a]).any() and (cloud[:, a] == np.inf).any() and (cloud[:, a] == -np.inf).any()
        assert all(med.cube_of_point(p) is None for p in cloud[nf]) and all(med.cube_of_point(p) is not None for p in cloud[~nf][::50])
    assert np.isfinite(fam.probes).all()


@pytest.mark.parametrize("name", list(med.ESCAPE_FAMILIES))
def test_cube_escape_centroid_leaves_its_cube(oracle, name):
    fam = med.family(name)
    leaf, face, sgn, cent = fam.plane_res, fam.info["face"], fam.info["sign"], fam.info["centroid"]
    om = oracle.OracleMap(plane_res=leaf, line_res=leaf / 2)
    assert om.add_surf(fam.clouds[0]) == med.ESCAPE_N
    exp = om.export()
    assert len(exp) == 1 and np.array_equal(_bits(exp[0]), _bits(cent)), "one centroid, the sequential float sum"
    beyond = (float(cent[0]) - face) * sgn
    print(f"{name}: centroid x = {cent[0]!r}, {beyond:.3f} m = {beyond / leaf:.1f} leaves beyond the face {face}")
    assert beyond > 2 * leaf, "the precondition of this family: more than two leaves outside its cube"
    home, across = med.cube_of_point(fam.clouds[0][0]), med.cube_of_point(cent)
    assert home != across and abs(home[0] - across[0]) == 1
    # a k = 1 probe inside the cube finds it; one in the cube across the face, right next to it, finds nothing
    f, nbr, d2, _, cube = om.knn(np.array([fam.info["inside"], cent]), 1, use_grid=0)
    assert f[0] and np.array_equal(nbr[0, 0], cent) and cube[0] == med.cube_linear(home) and not f[1]
    # it survives the second insert (its leaf receives nothing) ...
    om.add_surf(fam.clouds[1])
    assert (_bits(om.export()) == _bits(cent)).all(1).sum() == 1
    cubes = _oracle_cubes(om)
    assert (_bits(cubes[med.cube_linear(home)]) == _bits(cent)).all(1).sum() == 1
    # ... and the third, whose 50 points share its LEAF but lie across the face: VoxelGrid runs per cube, so the centroid stays
    # where it is and the cube across the face gains one point in the same leaf (no merge: the filter of LocalMap.h:622-640
    # never looks across a face)
    n_before = om.size()
    assert om.add_surf(fam.clouds[2]) == 50
    cubes = _oracle_cubes(om)
    assert om.size() == n_before + 1
    assert (_bits(cubes[med.cube_linear(home)]) == _bits(cent)).all(1).sum() == 1
    new = cubes[med.cube_linear(across)]
    same_leaf = (med.leaf_index(new, leaf) == med.leaf_index(cent, leaf)).all(1)
    assert same_leaf.sum() == 1 and np.array_equal(_bits(new[same_leaf][0]), _bits(med.float_centroid(fam.clouds[2])))
    # the probes at the end: full lists without ties
    found, _, d2, _, _ = om.knn(fam.probes, 6, use_grid=0)
    f = found.astype(bool)
    assert f.all() and (d2[:, 5] < 1e30).all() and (np.diff(d2, axis=1) > 0).all()
    for a, b in zip(om.knn(fam.probes, 5, use_grid=1)[:3], om.knn(fam.probes, 5, use_grid=0)[:3]):
        assert np.array_equal(a, b), (name, "grid search against brute force")


@pytest.mark.parametrize("name", list(med.PREFILTER))
def test_prefilter_clouds(oracle, name):
    pc = med.prefilter_cloud(name)
    cloud = pc.cloud
    dims = med.bounding_box_leaves(cloud, pc.plane_res)
    product = dims[0] * dims[1] * dims[2]
    got = oracle.voxel_grid(cloud, pc.plane_res)
    print(f"{name}: {len(cloud)} points, bounding box {dims} leaves = {product} ({'over' if product > med.INT32_MAX else 'under'} INT32_MAX), {len(got)} out")
    assert (product > med.INT32_MAX) == (name in med.PASS_THROUGH)
    if name in med.PASS_THROUGH:
        assert np.array_equal(_bits(got), _bits(cloud)), "the cloud passes through unchanged"
        if name != "box_1291":
            assert np.array_equal(_bits(oracle.voxel_grid(cloud, 0.2)), _bits(cloud))
    if name.startswith("box"):
        side = pc.info["side"]
        assert dims == (side, side, side) and (side ** 3 > med.INT32_MAX) == (side == 1291) and 1290 ** 3 < med.INT32_MAX < 1291 ** 3
        assert (len(got) < len(cloud)) == (side == 1290)
    if name == "long_leaves":
        sizes = med.leaf_sizes(cloud, pc.plane_res)
        print(f"{name}: {int((sizes > 64).sum())} leaves of more than 64 points, {int((sizes <= 64).sum())} shorter")
        assert (sizes > 64).sum() == 4200 > 4096 and (sizes <= 64).sum() == 2000 and len(got) == 6200
        return  # (too large for the plain loop)
    if name == "leaves_of_64":
        sizes = med.leaf_sizes(cloud, pc.plane_res)
        assert all((sizes == m).sum() == 5 for m in (63, 64, 65, 66))
    if name.startswith("leaf_faces"):
        assert len(cloud) > 300 and len(got) < len(cloud)
    assert np.array_equal(_bits(got), _bits(med.voxel_grid(cloud, pc.plane_res)))


def test_the_restatements_on_hand_checked_values():
    assert [med.cube_coord(c) for c in (0.0, 24.99, 25.0, -25.0, -25.01, -75.0, -75.01, 75.0)] == [0, 0, 1, 0, -1, -2, -2, 2]
    assert med.cube_coord(float("nan")) is None and med.cube_coord(float("inf")) is None and med.cube_coord(float("-inf")) is None
    assert med.origin_after_set(med.WINDOW_T) == (-3, 2, 0) and med.shift((-3, 2, 0), med.WINDOW_T) == ((0, 5, 3), (3, 3, 3))
    assert med.shift(med.DEFAULT_ORIGIN, (0.0, 0.0, 0.0)) == (med.DEFAULT_ORIGIN, (10, 10, 5))
    # two leaves, three points: sums in arrival order, leaves in ascending (z, y, x)
    out = med.voxel_grid(np.array([[0.3, 0.1, 0.1], [0.1, 0.1, 0.1], [0.35, 0.15, 0.1]], np.float32), 0.2)
    a, b = np.float32(0.3), np.float32(0.35)
    assert out.tolist() == [[np.float32(0.1)] * 3, [(a + b) / np.float32(2), (np.float32(0.1) + np.float32(0.15)) / np.float32(2), np.float32(0.1)]]
    assert med.leaf_index(np.float32(-0.0), 0.2) == 0 and med.leaf_index(med.down(0.0), 0.2) == -1


def test_origin_and_shift_restated_on_cube_faces(oracle):
    om = oracle.OracleMap(plane_res=0.2)
    for x in med.CUBE_FACES:
        for y in (-75.0, 25.0, 75.0):
            for z in med.Z_FACES:
                for t in ((x, y, z), (float(med.up(x)), float(med.down(y)), float(med.up(z))), (np.nextafter(x, -np.inf), np.nextafter(y, np.inf), z)):
                    t = np.array(t)
                    o = med.origin_after_set(t)
                    assert list(om.set_origin(t)) == list(o)
                    o2, pos = med.shift(o, t)
                    assert list(om.shift(t)) == list(pos) and list(om.origin()) == list(o2)
                    o3, pos = med.shift(o2, t + np.array([400.0, -250.0, 100.0]))
                    assert list(om.shift(t + np.array([400.0, -250.0, 100.0]))) == list(pos) and list(om.origin()) == list(o3)
