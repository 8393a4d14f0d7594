"""Sites for the bounded full pass of knn_plane_kernel (test infrastructure, beside knn_edge_data.py):

  bounded()     the FULL pass of a lane that comes out of the near pass with five exact neighbours searches the ball of its exact 5th
                distance (r_lane) instead of the gate ball.  Every site is ONE chunk -- the queries of one half-cell octant of one map
                cell -- built relative to the faces of its near block (the cells h .. h + 1 per axis around the upper octant of cell h):
                  a        a query 0.40 m from the low faces of its near block, four points within 0.2 m, a fifth INSIDE the block at
                           0.45 m and a sixth just across the x face at 0.42 m: outside the near block, it belongs into the list
                  b_lo/hi  the outside point at exactly the inside fifth's float d2 (mirror images on a 2^-10 grid), once in a cell that
                           precedes the fifth's in the canonical order and once in one that follows it
                  c_in     the outside point between sqrt(d5) and r_lane = sqrt(d5) * 1.0005 + 1e-4 (scanned, not in the list)
                  c_out    the outside point just beyond r_lane (not scanned, not in the list)
                  d        three points in the near block, four more 0.6 .. 0.7 m away across its faces: no fifth after the near pass,
                           the bound is the gate radius
                  e_out/in a fifth neighbour beyond the gate, across the face / inside the near block: TOO_FAR
                  f        cell 0 of cube (1, 0, 0): the ball of the 5th distance crosses the cube face x = 25, nearer points lie in cube
                           (0, 0, 0) and are not eligible
                  g        two kinds of query in one chunk, 0.08 m apart, that leave the near pass with 5th distances 0.52 and 0.44 m (one
                           group, two radii)
                each of them as an ordinary chunk (40 queries), a split chunk (24) and a light chunk (12).  The special queries are copies of
                the site's query, jittered by up to `jitter`; a and c are padded with EASY queries (around a corner of eight voxel
                leaves near the far corner of the octant, eight map points within 4 cm of them: the near pass certifies them).
Nothing here reads anything outside tests/."""
import numpy as np

import knn_edge_data as ked

f32, f64 = np.float32, np.float64
PLANE_RES = 0.2
NC, CELL = ked.grid_cells(PLANE_RES)       # 64 cells of 0.78125 m
R_NEAR = 0.5 * CELL                        # the near pass certifies nothing beyond it
GATE = f32(3) * f32(PLANE_RES)             # d2[4] > GATE: TOO_FAR
G = 2.0 ** -10
CHUNK_CLASSES = (("ordinary", 40, 8), ("split", 24, 6), ("light", 12, 4))  # (name, queries of the chunk, special queries among them)


def r_gate():
    """the kernel's gate radius, in its float arithmetic"""
    return f32(f32(np.sqrt(GATE)) * f32(1.0005) + f32(1e-4))


def r_lane(d5):
    """radius of the bounded full pass for a near-pass 5th distance d5 (float d2; inf: no fifth), in the kernel's float arithmetic"""
    d5 = np.asarray(d5, f64)
    with np.errstate(invalid="ignore"):
        r = (np.sqrt(np.where(np.isfinite(d5), d5, 0.0).astype(f32)) * f32(1.0005) + f32(1e-4)).astype(f32)
    return np.where(np.isfinite(d5), np.minimum(r, r_gate()), r_gate()).astype(f32)


def _snap(v):
    return np.round(np.asarray(v, f64) / G) * G


def _unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v)


def easy_homes():
    """home cells (per axis) that have a corner of voxel leaves 0.70 .. 0.745 m above their low face: the easy queries sit around it"""
    out = []
    for h in range(3, NC - 8):
        off = np.ceil((h * CELL + 0.70) / PLANE_RES - 1e-9) * PLANE_RES - h * CELL
        if off <= 0.745:
            out.append((h, off))
    return out


class _Builder:
    def __init__(self):
        self.used, self.mp, self.qs, self.sites = set(), [], [], []

    def free(self, p):
        return tuple(ked._leaf(np.asarray(p, f32), PLANE_RES)) not in self.used

    def add(self, p):
        p = np.asarray(p, f32)
        assert self.free(p), ("two map points in one voxel leaf", p)
        self.used.add(tuple(ked._leaf(p, PLANE_RES)))
        self.mp.append(p)
        return len(self.mp) - 1

    def near(self, s, n, radius):
        """n points at `radius` from s, in leaves of their own"""
        got = []
        for u in ked._sphere(48):
            p = s + _snap(radius * u)
            if self.free(p):
                got.append(self.add(p))
            if len(got) == n:
                return got
        raise AssertionError("no room for the near points")


def _site(b, rng, kind, cls, cube, h, spec):
    """one chunk; returns nothing, appends to the builder.  spec: dict(s_off, near=(n, radius), inside=[(dist, dir)], outside=[(dist, dir, snap)],
    jitter, easy (bool), second=(offset of the second kind of query, its near radius, its fifth's distance) or None)"""
    cname, n_q, n_special = cls
    cube, h = np.asarray(cube, f64), np.asarray(h, f64)
    mn = cube * ked.CUBE - 25.0
    base = mn + h * CELL
    s = _snap(base + np.asarray(spec["s_off"]))
    roles = {}
    roles["near"] = b.near(s, *spec["near"])
    roles["inside"] = [b.add(s + (_snap(d * _unit(u)) if sn else d * _unit(u))) for d, u, sn in spec.get("inside", ())]
    roles["outside"] = []
    for d, u, sn in spec.get("outside", ()):  # (a leaf already taken: the mirror image in y, in z, in both)
        for flip in ((1, 1, 1), (1, -1, 1), (1, 1, -1), (1, -1, -1)):
            p = s + (_snap(d * _unit(u)) if sn else d * _unit(u)) * np.array(flip)
            if b.free(p):
                break
        roles["outside"].append(b.add(p))
    centres = [s]
    if spec.get("second") is not None:  # a second kind of query that shares the site's points: special queries alternate between the two
        centres.append(_snap(s + np.asarray(spec["second"])))
    n_easy = n_q - n_special if spec.get("easy") else 0
    q = []
    for i in range(n_q - n_easy):
        c = centres[i % len(centres)]
        q.append(c if i < len(centres) else c + spec["jitter"] * rng.uniform(-1, 1, 3))
    if n_easy:
        offs = dict(easy_homes())
        ce = base + np.array([offs[int(v)] for v in h])
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    b.add(ce + 0.02 * np.array([sx, sy, sz]))
        q += [ce + rng.uniform(-0.015, 0.015, 3) for _ in range(n_easy)]
    q = np.array(q).astype(f32)
    half = np.floor((q.astype(f64) - mn) / (CELL / 2)).astype(np.int64)
    assert (half == 2 * h.astype(np.int64) + 1).all(), (kind, cname, "every query in the upper octant of the home cell")
    b.sites.append(dict(name=f"{kind}/{cname}", kind=kind, cls=cname, cube=tuple(int(v) for v in cube), home=tuple(int(v) for v in h),
                        first_query=sum(map(len, b.qs)), n_queries=len(q), n_special=len(q) - n_easy, roles=roles))
    b.qs.append(q)


_X_OUT = (-1.0, 0.05, 0.03)   # across the low x face of the near block
_IN5 = (1.0, 0.1, 0.1)        # into the block

BOUNDED_KINDS = {
    "a": dict(s_off=(0.40, 0.40, 0.40), near=(4, 0.15), inside=[(0.45, _IN5, True)], outside=[(0.42, _X_OUT, True)], jitter=2e-3, easy=True),
    # mirror images in x: the same float d2 from the site's own query; `lo`: the outside point's cell (x cell h - 1, same y, z) precedes the
    # fifth's (x cell h + 1); `hi`: the outside point one z cell UP (z cell h + 1), the fifth one down (z cell h)
    "b_lo": dict(s_off=(0.40, 0.40, 0.40), near=(4, 0.15), inside=[(1.0, (0.45, 0.0625, 0.03125), True)], outside=[(1.0, (-0.45, 0.0625, 0.03125), True)], jitter=1e-5),
    "b_hi": dict(s_off=(0.40, 0.40, 0.60), near=(4, 0.15), inside=[(1.0, (0.40625, 0.0625, -0.25), True)], outside=[(1.0, (-0.40625, 0.0625, 0.25), True)], jitter=1e-5),
    "c_in": dict(s_off=(0.40, 0.40, 0.40), near=(4, 0.15), inside=[(0.45, _IN5, False)], outside=[(0.45015, _X_OUT, False)], jitter=1e-5, easy=True),
    "c_out": dict(s_off=(0.40, 0.40, 0.40), near=(4, 0.15), inside=[(0.45, _IN5, False)], outside=[(0.4506, _X_OUT, False)], jitter=1e-5, easy=True),
    "d": dict(s_off=(0.40, 0.58, 0.58), near=(3, 0.15), outside=[(0.62, (-1.0, 0.3, 0.2), True), (0.65, (-1.0, -0.3, 0.25), True), (0.68, (-1.0, 0.25, -0.3), True),
                                                             (0.70, (-1.0, -0.2, -0.3), True)], jitter=2e-3),
    "e_out": dict(s_off=(0.40, 0.58, 0.58), near=(4, 0.15), outside=[(0.80, _X_OUT, True)], jitter=2e-3),
    "e_in": dict(s_off=(0.40, 0.58, 0.58), near=(4, 0.15), inside=[(0.80, _IN5, True)], jitter=2e-3),
    "f": dict(s_off=(0.40, 0.58, 0.58), near=(4, 0.15), inside=[(0.45, _IN5, True)], outside=[(0.42, _X_OUT, True), (0.44, (-1.0, -0.3, 0.25), True)], jitter=2e-3),
    # the second kind of query 0.08 m further into the block: its fifth is the inside point at 0.44 m, the first kind's the outside one at 0.42 m
    # (with 0.52 m as the 5th distance the near pass leaves it)
    "g": dict(s_off=(0.40, 0.58, 0.58), near=(4, 0.15), inside=[(0.52, (1.0, 0.0, 0.0), True)], outside=[(0.42, _X_OUT, True)], jitter=1e-3,
              second=(0.08, 0.0, 0.0)),
}


def _spec(kind):
    sp = dict(BOUNDED_KINDS[kind])
    if kind.startswith("b_"):  # (the offsets are given in metres, not as distance and direction: on the 2^-10 grid as they stand)
        sp["inside"] = [(np.linalg.norm(u), u, True) for _, u, _ in sp["inside"]]
        sp["outside"] = [(np.linalg.norm(u), u, True) for _, u, _ in sp["outside"]]
    return sp


def bounded(seed=21):
    rng = np.random.default_rng(seed)
    b = _Builder()
    homes = [h for h, _ in easy_homes()]
    assert len(homes) >= 6, homes
    far = [h for i, h in enumerate(homes) if i == 0 or h - homes[i - 1] > 4]   # one of every run of adjacent cells: sites at least 9 cells apart
    spots = [(hx, hy, hz) for hz in far[:2] for hy in far for hx in far]
    assert len(spots) >= 3 * (len(BOUNDED_KINDS) - 1), (far, len(spots))
    k = 0
    for kind in BOUNDED_KINDS:
        for cls in CHUNK_CLASSES:
            if kind == "f":
                cube, h = (1, 0, 0), (0, 8 + 6 * CHUNK_CLASSES.index(cls), 30)
            else:
                cube, h = (0, 0, 0), spots[k]
                k += 1
            _site(b, rng, kind, cls, cube, h, _spec(kind))
    # the second registration of the binned-ahead recipe (knn_edge_data.xruns): a patch far away
    pitch = PLANE_RES
    patch = ked._grid(ked._centres(-3 * pitch, 3 * pitch, pitch), ked._centres(150.0 - 3 * pitch, 150.0 + 3 * pitch, pitch), ked._centres(50.0 - 3 * pitch, 50.0 + 3 * pitch, pitch))
    n_site_points = len(b.mp)
    mp = np.concatenate([np.array(b.mp, f32), patch.astype(f32)])
    g = np.arange(-20.0, 20.0, 0.8)
    scan_a = ked._grid(g, g, np.array([-50.8, -50.0, -49.2])).astype(f32)
    return ked.Family("bounded_full_pass", mp, np.concatenate(b.qs), PLANE_RES, sites=b.sites, n_site_points=n_site_points, scan_a=scan_a,
                      pose_a=ked.XRUNS_POSE_A, aim="bounded")


def near_block_fifth(fam, exp):
    """per query of the family: float d2 of the 5th nearest map point among those of its NEAR block (cells h .. h + 1 of its own cube;
    inf with fewer than five) -- what the near pass leaves in the lane -- and the number of near-block points"""
    q = fam.queries
    qc, pc = ked.cube_of(q), ked.cube_of(exp)
    qcell, pcell = ked.cell_of(q, PLANE_RES), ked.cell_of(exp, PLANE_RES)
    d5 = np.full(len(q), np.inf)
    cnt = np.zeros(len(q), np.int64)
    for i in range(len(q)):
        m = (pc == qc[i]).all(1) & (pcell >= qcell[i]).all(1) & (pcell <= qcell[i] + 1).all(1)
        dd = np.sort(ked.d2_ref(q[i], exp[m]))
        cnt[i] = len(dd)
        if len(dd) >= 5:
            d5[i] = dd[4]
    return d5, cnt


def canonical_order(map_points, plane_res=PLANE_RES):
    """the map in the order the device keeps it (and export_map() lists it) inside a cube: by cell, z-major, then y, then x; points of a
    cell in the order given (test sites hold at most one point of interest per cell).  Cubes in lexicographic order -- enough for sites
    whose ties lie inside one cube."""
    cu, ce = ked.cube_of(map_points), ked.cell_of(map_points, plane_res)
    key = ((cu[:, 0] * 100 + cu[:, 1]) * 100 + cu[:, 2]) * 10 ** 7 + (ce[:, 2] * NC + ce[:, 1]) * NC + ce[:, 0]
    return map_points[np.argsort(key, kind="stable")]


def _row_of(exp, p):
    hit = np.nonzero((exp.view(np.uint32) == np.asarray(p, np.float32).view(np.uint32)).all(1))[0]
    assert len(hit) == 1
    return int(hit[0])


def check_sites(fam, exp, ref):
    """every site IS what its name says, judged by the brute force on the exported map (the canonical order)"""
    found, idx, d2, nbr, tail = ref
    d5_near, n_near = near_block_fifth(fam, exp)
    rl = r_lane(d5_near).astype(np.float64)
    gate = np.float64(GATE)
    seen, orders = set(), []
    for s in fam.info["sites"]:
        q0, ns = s["first_query"], s["n_special"]
        sp = slice(q0, q0 + ns)                      # the special queries
        easy = slice(q0 + ns, q0 + s["n_queries"])   # the easy ones (certified by the near pass: 5th distance well inside half a cell)
        kind, what = s["kind"], s["name"]
        row = lambda role, k=0: _row_of(exp, fam.map_points[s["roles"][role][k]])
        assert found[sp].all() and found[easy].all(), what
        assert (np.sqrt(d2[easy, 4].astype(np.float64)) < 0.2).all(), (what, "easy queries")
        # the near pass cannot finish a special query: fewer than five points in its near block, or the fifth of them beyond half a cell
        assert (np.sqrt(d5_near[sp]) > R_NEAR).all(), (what, "every special query goes to the full pass")
        if kind in ("a", "b_lo", "b_hi", "c_in", "c_out", "g"):
            assert (d2[sp, 4].astype(np.float64) <= gate).all() and (n_near[sp] >= 5).all(), (what, "five neighbours inside the gate, a fifth after the near pass")
            assert (rl[sp] < 0.6).all(), (what, "the bound is well below the gate radius")
        if kind in ("a", "g"):
            first = slice(q0, q0 + ns, 2) if kind == "g" else sp   # (g: every other special query is of the second kind)
            assert (idx[first] == row("outside")).any(1).all(), (what, "the point across the face belongs into every list")
            assert not (idx[first] == row("inside")).any(), (what, "and the fifth of the near block does not")
        if kind == "g":
            second = slice(q0 + 1, q0 + ns, 2)
            assert (idx[second, 4] == row("inside")).all(), (what, "the second kind's fifth is the inside point")
            a, b = np.sqrt(d5_near[first]), np.sqrt(d5_near[second])
            assert (a > 0.5).all() and (b < 0.46).all(), (what, "two 5th distances in one group", a, b)
        if kind in ("b_lo", "b_hi"):
            i_in, i_out = row("inside"), row("outside")
            dd = ked.d2_ref(fam.queries[q0], exp[[i_in, i_out]])
            assert dd[0] == dd[1] == d2[q0, 4], (what, "the outside point at exactly the inside fifth's float d2, both at rank 5", dd, d2[q0])
            assert idx[q0, 4] == min(i_in, i_out) and max(i_in, i_out) not in idx[q0], (what, "the canonical index decides")
            orders.append(i_out < i_in)
        if kind == "c_in":
            d_out = np.sqrt(np.float64(ked.d2_ref(fam.queries[q0], exp[[row("outside")]])[0]))
            assert np.sqrt(np.float64(d5_near[q0])) < d_out < rl[q0], (what, "between sqrt(d5) and r_lane", np.sqrt(d5_near[q0]), d_out, rl[q0])
            assert not (idx[sp] == row("outside")).any(), what
        if kind == "c_out":
            d_out = np.sqrt(np.float64(ked.d2_ref(fam.queries[q0], exp[[row("outside")]])[0]))
            assert rl[q0] < d_out < rl[q0] + 1e-3, (what, "just beyond r_lane", d_out, rl[q0])
            assert not (idx[sp] == row("outside")).any(), what
        if kind == "d":
            assert (n_near[sp] == 3).all() and np.isinf(d5_near[sp]).all() and (rl[sp] == r_gate()).all(), (what, "no fifth after the near pass: gate radius")
            far = np.sqrt(d2[sp, 3:5].astype(np.float64))
            assert (far > 0.6).all() and (far < 0.7).all() and (d2[sp, 4] <= gate).all(), (what, far.min(), far.max())
        if kind in ("e_out", "e_in"):
            assert (d2[sp, 4].astype(np.float64) > gate).all() and (d2[sp, 3].astype(np.float64) < 0.04).all(), (what, "a fifth neighbour beyond the gate")
            assert (n_near[sp] == (5 if kind == "e_in" else 4)).all(), what
        if kind == "f":
            pts = fam.map_points[s["roles"]["outside"]]
            assert (ked.cube_of(pts) != ked.cube_of(fam.queries[q0])).any(1).all(), (what, "the nearer points lie in the other cube")
            assert (ked.d2_ref(fam.queries[q0], pts) < d2[q0, 4]).all() and (d2[sp, 4] <= gate).all(), (what, "and are nearer than the fifth")
            assert (np.sqrt(d5_near[sp]) + 0.0 > fam.queries[sp, 0].astype(np.float64) - 25.0).all(), (what, "the ball of the 5th distance crosses the cube face")
        seen.add((kind, s["cls"]))
    assert seen == {(k, c[0]) for k in BOUNDED_KINDS for c in CHUNK_CLASSES}, "no site is skipped"
    assert sorted(orders) == [False] * 3 + [True] * 3, ("the tie in both index orders", orders)
    return len(fam.info["sites"])
