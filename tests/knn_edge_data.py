"""Path-directed inputs for the exact 5-NN search and a plain numpy reference of it (test infrastructure).

The contract (include/so_icp.h): the five nearest map points INSIDE the query's 50 m cube, ascending d2, ties by ascending
canonical index; d2 in the reference's arithmetic (float differences, fp64 squares and sum, narrowed to float).

Every family is a seeded, deterministic function that returns a `Family`: map points that survive the map's voxel filter
unchanged (one point per planeRes leaf), queries, planeRes.  The families aim at the branches of the device sweeps that noisy
surfaces never reach:

  ties_*      exact ties in float d2 (lattices at the leaf centres; a power-of-two pitch keeps every symmetric tie exact):
              eight and more equal distances around rank 5 -- no approximate key can order them, no pass can certify them
  near_ties   twelve points on a shell whose d2 differ by 0 .. ~700 ulps (all inside the selection's error bound), ranks 5 and
              6 exactly one ulp apart
  dense       planeRes 0.1, sites whose 2 x 2 x 2 cell block holds a KNOWN number of candidates: around the 2048 limit of the
              key's index field, around the 384-candidate tile and its multiples, around the 96 candidates / 1024 block points
              of a packed row
  faces       queries within 1e-3 m of a cube face, on it, at cube edges and corners, with the nearest map points across the
              face; cubes of 1 .. 6 points; the last cube of the 21 x 21 x 11 window and a query beyond it; at planeRes 0.2, 0.4
              (45 cells of 50/45 m) and 0.8 (32 cells)
  gate_edge   the neighbour-distance gate d2[4] > 3 * planeRes: per direction and placement of the query a fifth neighbour exactly ON
              the gate (or at the last float configuration inside it) and the float-adjacent one outside; planeRes 0.2, 0.33, 0.4, 0.8
  cell_faces  map points and queries on interior cell faces of the grids whose cell is no binary fraction (57 and 45 cells per cube)
  nonfinite_rows  NaN, +-inf and 1e12 written into rows of a scan (a function of a scan, not a family)
  xruns       scans for the binned-ahead path: chunks of queries from all over a lattice (more than 16 / 32 x-runs) and with lanes in
              eight cubes
  boundary_block  one chunk whose near block begins at the cube's own face (not a member of FAMILIES: one dedicated device test)

Nothing here reads anything outside tests/ and nothing depends on the oracle or on the product."""
import numpy as np

CUBE = 50.0
K = 5
FLT_MAX = np.finfo(np.float32).max


class Family:
    def __init__(self, name, map_points, queries, plane_res, **info):
        self.name = name
        self.map_points = np.ascontiguousarray(map_points, dtype=np.float32)
        self.queries = np.ascontiguousarray(queries, dtype=np.float32)
        self.plane_res = float(plane_res)
        self.info = info
        leaf = np.floor(self.map_points * np.float32(np.float32(1.0) / np.float32(plane_res))).astype(np.int64)
        assert len(np.unique(leaf, axis=0)) == len(leaf), f"{name}: two map points share a voxel-filter leaf"


# ------------------------------------------------------------------------------------------------------------------------
# the plain reference
# ------------------------------------------------------------------------------------------------------------------------
def cube_of(p):
    return np.floor((np.asarray(p, np.float32).astype(np.float64) + 25.0) / CUBE).astype(np.int64)


def d2_ref(q, pts):
    """float differences, fp64 squares and sum, narrowed to float: q [3] or [n, 3] against pts [n, 3]"""
    d = (np.asarray(q, np.float32) - np.asarray(pts, np.float32)).astype(np.float32).astype(np.float64)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def cell_counts(map_points, queries):
    """map points in the query's cube, per query"""
    mc, qc = cube_of(map_points), cube_of(queries)
    cubes, inv, cnt = np.unique(mc, axis=0, return_inverse=True, return_counts=True)
    look = {tuple(c): n for c, n in zip(cubes, cnt)}
    return np.array([look.get(tuple(c), 0) for c in qc])


def brute_knn(map_points, queries, k=K, n_tail=0):
    """Exhaustive search per query over the map points of its cube, lexsort by (d2, index in `map_points` order).
    Returns found [nq] bool, idx [nq, k] (index into map_points), d2 [nq, k] float32, nbr [nq, k, 3], and -- with n_tail -- the
    sorted d2 of the first k + n_tail candidates [nq, k + n_tail] (inf where the cube holds fewer).
    A cube with fewer than k points leaves what the reference's result set leaves: unfilled slots name the cube's first point
    with d2 0, the last slot carries FLT_MAX."""
    mp = np.ascontiguousarray(map_points, np.float32); q = np.ascontiguousarray(queries, np.float32)
    nq = len(q)
    found = np.zeros(nq, bool); idx = np.zeros((nq, k), np.int64); d2 = np.zeros((nq, k), np.float32)
    tail = np.full((nq, k + n_tail), np.inf, np.float64)
    mc, qc = cube_of(mp), cube_of(q)
    cubes, minv = np.unique(mc, axis=0, return_inverse=True)
    minv = minv.reshape(-1)
    look = {tuple(c): i for i, c in enumerate(cubes)}
    qcube = np.array([look.get(tuple(c), -1) for c in qc])
    for ci in np.unique(qcube):
        if ci < 0:
            continue
        members = np.nonzero(minv == ci)[0]  # ascending = the order of map_points
        cand = mp[members]
        qs = np.nonzero(qcube == ci)[0]
        for s in range(0, len(qs), 128):
            qi = qs[s:s + 128]
            dd = d2_ref(q[qi][:, None, :], cand[None, :, :])  # [nqi, nc]
            key = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(members), dtype=np.uint64)[None, :]
            key.sort(axis=1)
            m = min(k, len(members))
            loc = (key[:, :m] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            found[qi] = True
            idx[qi] = members[0]
            idx[qi, :m] = members[loc]
            d2[qi, :m] = (key[:, :m] >> np.uint64(32)).astype(np.uint32).view(np.float32)
            if m < k:
                d2[qi, k - 1] = FLT_MAX
            mt = min(k + n_tail, len(members))
            tail[qi, :mt] = (key[:, :mt] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    nbr = mp[idx] if len(mp) else np.zeros((nq, k, 3), np.float32)
    nbr[~found] = 0
    return (found, idx, d2, nbr, tail) if n_tail else (found, idx, d2, nbr)


# ------------------------------------------------------------------------------------------------------------------------
# 1. exact ties
# ------------------------------------------------------------------------------------------------------------------------
def _centres(lo, hi, pitch):
    """leaf centres (i + 0.5) * pitch inside [lo, hi)"""
    i = np.arange(int(np.floor(lo / pitch)), int(np.ceil(hi / pitch)))
    c = (i + 0.5) * pitch
    return c[(c >= lo) & (c < hi)]


def _grid(xs, ys, zs):
    g = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
    return g


def _tie_queries(anchors, pitch, rng, n_each):
    """at lattice points, edge midpoints, face centres, cell centres -- and a fixed height (a quarter pitch) above each of these"""
    out = []
    for shift in ((0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), (0.5, 0.5, 0), (0.5, 0, 0.5), (0, 0.5, 0.5), (0.5, 0.5, 0.5)):
        a = anchors[rng.choice(len(anchors), size=min(n_each, len(anchors)), replace=False)]
        base = a + np.array(shift) * pitch
        out += [base, base + np.array([0, 0, 0.25 * pitch])]
    return np.concatenate(out)


def ties_volume(pitch, seed=1):
    """a full lattice around the origin and one across the cube face x = 25"""
    rng = np.random.default_rng(seed)
    half = 9 * pitch
    a = _grid(_centres(-half, half, pitch), _centres(-half, half, pitch), _centres(-half, half, pitch))
    b = _grid(_centres(25 - half, 25 + half, pitch), _centres(3 - half, 3 + half, pitch), _centres(-half, half, pitch))
    mp = np.concatenate([a, b])
    inner = lambda g, c: g[(np.abs(g - c) < half - 2.5 * pitch).all(1)]
    q = np.concatenate([_tie_queries(inner(a, np.zeros(3)), pitch, rng, 150), _tie_queries(inner(b, np.array([25.0, 3.0, 0.0])), pitch, rng, 150)])
    return Family(f"ties_volume_{pitch}", mp, q, pitch, pitch=pitch, power_of_two=(pitch in (0.25, 0.125)), aim="fallback")


def ties_sheets(pitch, seed=2):
    """a floor and two walls, one leaf thick: above a cell centre of a sheet four equal distances, then eight"""
    rng = np.random.default_rng(seed)
    L = 24 * pitch
    u, v = _centres(-L, L, pitch), _centres(-L, L, pitch)
    z0 = _centres(-2.0, -2.0 + pitch, pitch)
    floor = _grid(u, v, z0)
    w = _centres(z0[0] + pitch, z0[0] + 20 * pitch, pitch)
    wall_x = _grid(_centres(-L - pitch, -L, pitch), v, w)
    wall_y = _grid(u, _centres(L, L + pitch, pitch), w)
    mp = np.concatenate([floor, wall_x, wall_y])
    sel = lambda g: g[rng.choice(len(g), size=160, replace=False)]
    fl = floor[(np.abs(floor[:, :2]) < L - 3 * pitch).all(1)]
    q = [_tie_queries(fl, pitch, rng, 160)]
    # beside the walls: the same pattern turned into the wall's plane
    wx = wall_x[(np.abs(wall_x[:, 1]) < L - 3 * pitch) & (wall_x[:, 2] > w[2]) & (wall_x[:, 2] < w[-3])]
    wy = wall_y[(np.abs(wall_y[:, 0]) < L - 3 * pitch) & (wall_y[:, 2] > w[2]) & (wall_y[:, 2] < w[-3])]
    for g, normal in ((wx, np.array([1.0, 0, 0])), (wy, np.array([0, -1.0, 0]))):
        for s1 in (0.0, 0.5):
            for s2 in (0.0, 0.5):
                base = sel(g) + np.array([0, 0, s2 * pitch]) + s1 * pitch * np.abs(np.cross(normal, [0, 0, 1.0]))
                q += [base, base + 0.25 * pitch * normal, base + 0.75 * pitch * normal]
    return Family(f"ties_sheets_{pitch}", mp, np.concatenate(q), pitch, pitch=pitch, power_of_two=(pitch in (0.25, 0.125)), aim="fallback")


# ------------------------------------------------------------------------------------------------------------------------
# 2. near-ties
# ------------------------------------------------------------------------------------------------------------------------
_G = 2.0 ** -18   # grid of the offsets: query on a 2^-10 grid (|q| < 32) + offset on this grid is exact in float
_C0 = 2.0 ** -9   # the small component: one grid step of it moves d2 by 2 * 2^-9 * 2^-18 = 2^-26 = one ulp of d2 in [0.125, 0.25)

# offsets of the twelve d2 from the smallest, in ulps: ranks 5 and 6 one ulp apart and tied with nothing (exact ties elsewhere),
# everything within 1e-5 (~670 ulps)
_NEAR_PATTERNS = (
    (0, 1, 2, 3, 4, 5, 8, 16, 64, 256, 512, 660),
    (0, 0, 3, 3, 7, 8, 9, 9, 40, 41, 300, 301),
    (0, 2, 2, 2, 3, 4, 5, 5, 5, 6, 100, 600),
    (0, 10, 20, 30, 40, 41, 42, 43, 44, 45, 46, 47),
)


def approx_d2_block_local(q, pts, plane_res):
    """The selection key's distance, restated: query and candidates relative to the centre of the lower cell of the query's near
    block (fp64 subtraction, narrowed), then (|c|^2 + |q|^2) - 2 q.c in fp32 with fused multiply-adds (each emulated by one fp64
    operation narrowed to float: the products of two floats are exact in fp64).  q [3], pts [n, 3] -> float32 [n]."""
    f32, f64 = np.float32, np.float64
    nc, cell = grid_cells(plane_res)
    cellf = f32(1.0 / (nc / CUBE))
    mn = cube_of(q).astype(f64) * CUBE - 25.0
    u = (np.asarray(q, f32).astype(f64) - mn).astype(f32)
    lo = np.maximum(0, np.floor((u - f32(0.5) * cellf) * f32(nc / CUBE)).astype(np.int64))
    o = mn + (lo.astype(f64) + 0.5) * f64(cellf)
    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    lq = (np.asarray(q, f32).astype(f64) - o).astype(f32)
    lc = (np.asarray(pts, f32).astype(f64) - o).astype(f32)
    sq = lambda v: fma(v[..., 2], v[..., 2], fma(v[..., 1], v[..., 1], (v[..., 0] * v[..., 0]).astype(f32)))
    qq, cc = sq(lq), sq(lc)
    m2q = (f32(-2.0) * lq).astype(f32)
    v = (cc + qq).astype(f32)
    for a in range(3):
        v = fma(np.broadcast_to(m2q[a], lc[:, a].shape), lc[:, a], v)
    return v


KEY_KEEP = np.uint32(0xFFFFF800)  # the key keeps the distance's high 21 bits; its low 11 carry the candidate's position


def _ulps_up(x, n):
    return (np.float32(x).view(np.uint32) + np.uint32(n)).view(np.float32)


def near_ties(seed=3):
    """One query per site, twelve map points around it at radius ~0.42 m (planeRes 0.2: inside the gate, each in a leaf of its own),
    their exact d2 tuned to base + pattern[k] ulps.  Each point has two large offset components and one of ~2^-9 m whose grid steps
    move d2 by one ulp.  A site is drawn again until the block-local fp32 distance (approx_d2_block_local) puts the exact 5th and 6th
    neighbour in the REVERSE of their exact order: every site holds such a pair."""
    rng = np.random.default_rng(seed)
    plane_res = 0.2
    mp, qs, want = [], [], []
    r = 0.42
    sites = [(x, y, z) for z in (-6.0, 0.0, 6.0) for x in np.arange(-20, 21, 4.0) for y in np.arange(-20, 21, 4.0)]
    for s, c in enumerate(sites):
        pat = _NEAR_PATTERNS[s % len(_NEAR_PATTERNS)]
        for _ in range(200):
            q = np.round((np.array(c) + rng.uniform(-0.5, 0.5, 3)) * 1024) / 1024
            ang = rng.uniform(0, 2 * np.pi) + np.arange(4) * (np.pi / 2) + rng.uniform(-0.25, 0.25, 4)
            offs = []
            for plane in range(3):  # four points near each coordinate plane through the query
                a, b = r * np.cos(ang + plane), r * np.sin(ang + plane)
                for t in range(4):
                    o = np.zeros(3)
                    o[(plane + 1) % 3], o[(plane + 2) % 3], o[plane] = a[t], b[t], _C0 * (1 if t % 2 else -1)
                    offs.append(np.round(o / _G) * _G)
            offs = np.array(offs)
            order = rng.permutation(12)  # which point gets which rank: unrelated to the order of insertion (= of the indices)
            base = d2_ref(q.astype(np.float32), (q + offs[order[0]]).astype(np.float32)[None])[0]
            ok = 0.125 < base < 0.24
            for kk in range(12):
                if not ok:
                    break
                o = offs[order[kk]]
                ax = int(np.argmin(np.abs(o)))
                target = _ulps_up(base, pat[kk])
                steps = np.arange(-1500, 1501)
                cand = np.repeat(o[None], len(steps), 0)
                cand[:, ax] = o[ax] + np.sign(o[ax]) * steps * _G
                dd = d2_ref(q.astype(np.float32), (q + cand).astype(np.float32))
                hit = np.nonzero(dd.view(np.uint32) == target.view(np.uint32))[0]
                if not len(hit):
                    ok = False
                    break
                offs[order[kk]] = cand[hit[0]]
            pts = (q + offs).astype(np.float32)
            if ok and np.array_equal(pts.astype(np.float64), q + offs) and \
                    len(np.unique(np.floor(pts * np.float32(5.0)).astype(np.int64), axis=0)) == 12:
                a = approx_d2_block_local(q.astype(np.float32), pts[order[4:6]], plane_res)
                if pat[5] > pat[4] and a[0] > a[1]:
                    break
        else:
            raise AssertionError(f"near_ties: site {s} could not be tuned")
        mp.append(pts); qs.append(q); want.append(pat)
    return Family("near_ties", np.concatenate(mp), np.array(qs), plane_res, patterns=np.array(want), aim="fallback")


# ------------------------------------------------------------------------------------------------------------------------
# 3. dense blocks
# ------------------------------------------------------------------------------------------------------------------------
def grid_cells(plane_res):
    """cells per cube and cell size of the product's grid (local_map.cpp cells_per_cube)"""
    r_max = np.sqrt(np.float64(np.float32(3) * np.float32(plane_res)))
    nc = int(min(64, max(1, np.floor(CUBE / (r_max * 1.005)))))
    return nc, CUBE / nc


# (candidates in the site's 2 x 2 x 2 block, queries of the site): a site of 40 queries is one ordinary chunk, one of 12 a light
# chunk (<= 16 queries: a packed row, or a wavefront split four ways without the packing)
DENSE_SITES = ((2047, 40), (2048, 40), (2049, 40), (3300, 40), (2047, 12), (2048, 12), (2049, 12), (3300, 12),   # the key's index field
               (383, 40), (384, 40), (385, 40), (767, 40), (768, 40), (769, 40), (1000, 40),                     # the tile and its refills
               (95, 12), (96, 12), (97, 12), (200, 12), (1023, 12), (1024, 12), (1025, 12))                      # a packed row's quarter, its block limit


def dense(seed=4, n_cubes=7, site_list=None, name="dense"):
    """planeRes 0.1, lattice pitch 0.1.  A site: home cell h, queries in the upper octant of h (every near ball then covers exactly
    the cells h .. h + 1 per axis), and as map the K lattice points of that block nearest to the queries' bounding box -- the block
    holds exactly K candidates before any filter.  For K <= 1000 all of them lie within the near radius of the box, so the candidate
    filter keeps all K."""
    rng = np.random.default_rng(seed)
    plane_res, pitch = 0.1, 0.1
    nc, cell = grid_cells(plane_res)
    cube_list = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (1, 1, 0), (-1, -1, 0)][:n_cubes]
    mp, qs, sites = [], [], []
    for cu in cube_list:
        mn = np.array(cu, float) * CUBE - 25.0
        homes = [(4 * i + 5, 4 * j + 5, 4 * k + 5) for i in range(3) for j in range(3) for k in range(3)]
        rng.shuffle(homes)
        for (kcount, nq), h in zip(site_list or DENSE_SITES, homes):
            h = np.array(h)
            lo, hi = mn + h * cell, mn + (h + 2) * cell
            g = _grid(_centres(lo[0] - pitch, hi[0] + pitch, pitch), _centres(lo[1] - pitch, hi[1] + pitch, pitch),
                      _centres(lo[2] - pitch, hi[2] + pitch, pitch)).astype(np.float32)
            c = np.floor((g.astype(np.float64) - mn) * (nc / CUBE)).astype(np.int64)  # cell of a map point: fp64 on its own coordinates
            g = g[((c >= h) & (c <= h + 1)).all(1)]
            t = rng.uniform(0.03, 0.97, (nq, 3)) if kcount > 300 else rng.uniform(0.35, 0.65, (nq, 3))
            q = (mn + (h + 0.5 + 0.5 * t) * cell).astype(np.float32)
            b0, b1 = q.min(0).astype(np.float64), q.max(0).astype(np.float64)
            e = np.maximum(np.maximum(b0 - g, g - b1), 0.0)
            dist = np.sqrt((e * e).sum(1))
            order = np.argsort(dist, kind="stable")
            assert len(g) >= kcount, (len(g), kcount)
            keep = np.sort(order[:kcount])
            if kcount <= 1000:
                assert dist[order[kcount - 1]] < 0.5 * cell - 1e-3, (kcount, nq, dist[order[kcount - 1]])
            mp.append(g[keep]); qs.append(q); sites.append((cu, tuple(h), kcount, nq))
    return Family(name, np.concatenate(mp), np.concatenate(qs), plane_res, sites=sites, aim="dense")


# ------------------------------------------------------------------------------------------------------------------------
# 4. cube faces and the window
# ------------------------------------------------------------------------------------------------------------------------
def _leaf(p, plane_res):
    """the voxel filter's leaf of a point (the expression the Family constructor asserts with)"""
    return np.floor(np.asarray(p, np.float32) * np.float32(np.float32(1.0) / np.float32(plane_res))).astype(np.int64)


def _first_per_leaf(points, plane_res):
    """drop every point whose leaf an earlier point of the list occupies (the order of the others is kept)"""
    _, first = np.unique(_leaf(points, plane_res), axis=0, return_index=True)
    return points[np.sort(first)]


def faces(plane_res=0.2, seed=5):
    """A site sits at a point c of a cube face, edge or corner: a lattice of 5 pitches (pitch = planeRes; 2 m at 0.2) around c, thinned
    out INSIDE the queries' own cube to the points at least 2.25 pitches (0.45 m at 0.2; Chebyshev) from c, so that the points across the
    face are the nearest ones.  The queries lie in one cube per site: the high side (on the face itself, one ulp, 1e-4 and 1e-3 beyond
    it) or the low side.  Lattice, thinning radius and the queries' tangential offsets scale with planeRes (s = planeRes / 0.2); the sites
    stay where they are, so at 0.4 and 0.8 their lattices overlap: every site's hole is cut out of every lattice and a leaf keeps the first
    point that falls into it.  At 0.2 neither does anything, and the first `n_map_v1` map points / `n_queries_v1` queries are the bytes
    the family had before it took planeRes.  Behind them: cubes of exactly 1, 2 and 3 points."""
    rng = np.random.default_rng(seed)
    pitch = plane_res
    s = plane_res / 0.2
    mp, qs = [], []
    f32 = np.float32

    def side_values(face, high):
        if high:
            return [f32(face), np.nextafter(f32(face), f32(np.inf)), f32(face + 1e-4), f32(face + 1e-3)]
        return [np.nextafter(f32(face), f32(-np.inf)), f32(face - 1e-4), f32(face - 1e-3)]

    site_list = []
    for y in (-14.0, -7.0, 0.0, 7.0, 14.0):  # faces x = +-25, y = +-25, both sides
        for face in (25.0, -25.0):
            for high in (True, False):
                site_list.append(({0: (face, high)}, np.array([face, y + (3.0 if high else 0.0), 1.0 + face / 50])))
                site_list.append(({1: (face, high)}, np.array([y + (3.0 if high else 0.0), face, -1.0 + face / 50])))
    for z in (-6.0, 6.0):  # the face z = +-25 is in reach of the window too (11 cubes deep)
        for high in (True, False):
            site_list.append(({2: (25.0, high)}, np.array([z, z + (2.0 if high else -2.0), 25.0])))
            site_list.append(({2: (-25.0, high)}, np.array([z, -z - (2.0 if high else -2.0), -25.0])))
    k = 0
    for hx in (True, False):  # cube edges and corners: every quadrant / octant at an edge piece / a corner of its own
        for hy in (True, False):
            site_list.append(({0: (25.0, hx), 1: (25.0, hy)}, np.array([25.0, 25.0, -9.0 + 6.0 * k])))
            site_list.append(({0: (-25.0, hx), 1: (25.0, hy)}, np.array([-25.0, 25.0, -9.0 + 6.0 * k])))
            k += 1
            for hz in (True, False):
                c = np.array([25.0 if hx else -25.0, -25.0 if hy else 25.0, 25.0 if hz else -25.0])
                site_list.append(({0: (c[0], hx), 1: (c[1], hy), 2: (c[2], hz)}, c))
    seen, holes = {}, []
    for axes, c in site_list:
        key = tuple(c)
        assert key not in seen, "every site has a lattice of its own"
        g = _grid(_centres(c[0] - 1.0 * s, c[0] + 1.0 * s, pitch), _centres(c[1] - 1.0 * s, c[1] + 1.0 * s, pitch),
                  _centres(c[2] - 1.0 * s, c[2] + 1.0 * s, pitch)).astype(np.float32)
        vals = [None, None, None]
        for a in range(3):
            if a in axes:
                vals[a] = side_values(*axes[a])
            else:
                vals[a] = [f32(c[a] + d * s) for d in (0.0, 0.1, -0.23) + tuple(rng.uniform(-0.3, 0.3, 1))]
        q = _grid(*vals).astype(np.float32)
        qcube = cube_of(q)
        assert (qcube == qcube[0]).all()
        seen[key] = g
        holes.append((qcube[0], c))
        qs.append(q)

    def thinned(g):
        for qcube, c in holes:
            g = g[~((cube_of(g) == qcube).all(1) & (np.abs(g.astype(np.float64) - c).max(1) < 0.45 * s))]
        return g

    mp += [thinned(g) for g in seen.values()]

    def small_cube(n, cx):
        pts = np.array([cx, 10.0, 0.0]) + s * (np.arange(n)[:, None] * np.array([0.25, 0.0, 0.0]) + np.array([[0, 0.3 * (i % 2), 0.3 * (i % 3)] for i in range(n)]))
        return [pts.astype(np.float32)], [(pts[:3] + s * np.array([0.05, 0.02, -0.04])).astype(np.float32),
                                          np.array([[cx + 0.6 * s, 10.0 + 0.1 * s, 0.2 * s], [cx - 3.0, 9.0, 0.0]], np.float32)]

    # cubes holding exactly 4, 5 and 6 points
    for n, cx in ((4, 150.0), (5, 200.0), (6, 250.0)):
        m_, q_ = small_cube(n, cx)
        mp += m_; qs += q_
    # the last cube of the window in x (cubes -10 .. 10 around a sensor at the origin: x in [-525, 525)) and beyond it
    edge = _grid(_centres(525.0 - 2.0 * s, 525.0, pitch), _centres(-1.0 * s, 1.0 * s, pitch), _centres(-1.0 * s, 1.0 * s, pitch)).astype(np.float32)
    edge = edge[edge[:, 0] < f32(525.0 - 0.05 * s)]
    mp.append(edge)
    eq = _grid([f32(525.0 - 1.0 * s), f32(525.0 - 0.1 * s), np.nextafter(f32(525.0), f32(-np.inf)), f32(525.0), f32(525.5), f32(-526.0)],
               [f32(0.0), f32(0.31 * s)], [f32(0.1 * s), f32(-0.45 * s)])
    qs.append(eq.astype(np.float32))
    # first and last cell of a cube, away from any site: the clamped neighbourhood over an ordinary lattice
    for cx in (-24.9, 24.9):
        g = _grid(_centres(cx - 1.0 * s if cx > 0 else -25.0, 25.0 if cx > 0 else cx + 1.0 * s, pitch), _centres(-19.0 - 1.0 * s, -19.0 + 1.0 * s, pitch),
                  _centres(4.0 - 1.0 * s, 4.0 + 1.0 * s, pitch))
        mp.append(thinned(g.astype(np.float32)))
        qs.append((np.array([cx, -19.0, 4.0]) + s * rng.uniform(-0.08, 0.08, (40, 3))).astype(np.float32))
    n_face = sum(len(q) for q in qs[:len(site_list)])
    n_map_v1, n_queries_v1 = sum(map(len, mp)), sum(map(len, qs))
    # cubes holding exactly 1, 2 and 3 points (behind everything the family had before)
    for n, cx in ((1, 300.0), (2, 350.0), (3, 400.0)):
        m_, q_ = small_cube(n, cx)
        mp += m_; qs += q_
    mp = np.concatenate(mp)
    if s != 1.0:
        mp = _first_per_leaf(mp, plane_res)
    name = "faces" if plane_res == 0.2 else f"faces_{plane_res}"
    return Family(name, mp, np.concatenate(qs), plane_res, n_face_queries=n_face, n_map_v1=n_map_v1, n_queries_v1=n_queries_v1, aim="faces")


def nearest_across(map_points, queries):
    """d2 to the nearest map point OUTSIDE the query's cube (inf if there is none within reach of this brute force)"""
    mp = np.asarray(map_points, np.float32); q = np.asarray(queries, np.float32)
    mc, qc = cube_of(mp), cube_of(q)
    out = np.full(len(q), np.inf)
    for i in range(len(q)):
        near = (np.abs(mp.astype(np.float64) - q[i].astype(np.float64)) < 2.0).all(1) & ~(mc == qc[i]).all(1)
        if near.any():
            out[i] = d2_ref(q[i], mp[near]).min()
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 5. chunks that are NOT compact: more than 16 / 32 x-runs, lanes of one chunk in several cubes
# ------------------------------------------------------------------------------------------------------------------------
XRUNS_POSE_A = np.array([0.0, 150.0, 100.0, 0, 0, 0, 1.0])


def xruns(seed=6):
    """A chunk is one half-cell octant under the pose the scan was BINNED with.  It stops being one only when the scan is binned ahead
    of its registration under another pose (so_icp_stage_scan): scan B is announced, registration A (pose XRUNS_POSE_A: 100 m up,
    where B lands in cubes without map points, so all of B shares the one "no cube" bucket and is cut into chunks of 64 in arrival
    order) bins it, and B's own registration sweeps those chunks under the identity, where their queries lie all over a lattice.
      queries[:n_one]   4 489 queries spread over 8 m inside ONE cube: any chunk spans more than 32 x-runs, the light chunk of 9 that
                        is left over more than 16
      queries[n_one:]   4 489 queries around the cube corner (25, 25, 25): every chunk has lanes in eight cubes
    scan_a: 7 500 points that under XRUNS_POSE_A lie 0.8 m apart in the cube of a small patch (each a light chunk of its own: the list
    does not fit the sweep's grid one chunk per wavefront, which is what keeps the packing of light chunks on for B)."""
    rng = np.random.default_rng(seed)
    plane_res, pitch = 0.2, 0.2
    c1, c2 = np.array([8.0, 8.0, 8.0]), np.array([25.0, 25.0, 25.0])
    lat = lambda c, h: _grid(_centres(c[0] - h, c[0] + h, pitch), _centres(c[1] - h, c[1] + h, pitch), _centres(c[2] - h, c[2] + h, pitch))
    patch = lat(np.array([0.0, 150.0, 50.0]), 0.6)
    mp = np.concatenate([lat(c1, 4.4), lat(c2, 4.4), patch]).astype(np.float32)
    n = 64 * 70 + 9
    q1 = (c1 + rng.uniform(-4.0, 4.0, (n, 3))).astype(np.float32)
    q2 = (c2 + rng.uniform(-4.0, 4.0, (n, 3))).astype(np.float32)
    g = np.arange(-20.0, 20.0, 0.8)
    scan_a = _grid(g, g, np.array([-50.8, -50.0, -49.2])).astype(np.float32)
    return Family("xruns", mp, np.concatenate([q1, q2]), plane_res, n_one=n, scan_a=scan_a, pose_a=XRUNS_POSE_A, aim="xruns")


def boundary_block(seed=7):
    """40 queries of ONE chunk (one half-cell octant) within 5 cm of the low x face of a cube, over a lattice that lies inside their
    cube only: the near block starts at cell 0, its low x face is the cube's boundary and has nothing of the cube behind it, every other
    face is 0.39 m or more away and the 5th neighbour at most ~0.3 m: the NEAR pass must certify every query."""
    rng = np.random.default_rng(seed)
    pitch = 0.2
    mp = _grid(_centres(-25.0, -23.0, pitch), _centres(4.0, 6.4, pitch), _centres(4.0, 6.4, pitch)).astype(np.float32)
    nc, cell = grid_cells(pitch)
    lo = (np.floor(30.2 / cell) + 0.5) * cell - 25.0  # lower end of the upper half of a cell, in y and in z
    q = np.c_[-25.0 + rng.uniform(1e-3, 0.05, 40), lo + rng.uniform(0.02, 0.5 * cell - 0.02, 40), lo + rng.uniform(0.02, 0.5 * cell - 0.02, 40)]
    return Family("boundary_block", mp, q.astype(np.float32), pitch, aim="cover")


# ------------------------------------------------------------------------------------------------------------------------
# 6. the neighbour-distance gate: d2[4] > 3 * planeRes (float product) rejects the query
# ------------------------------------------------------------------------------------------------------------------------
def cell_of(p, plane_res):
    """cell of a point inside its cube: the fp64 expression of locate (kernels.hip) / cell_coords (map_kernels.hip) on the point's
    own float coordinates"""
    nc, cell = grid_cells(plane_res)
    p64 = np.asarray(p, np.float32).astype(np.float64)
    mn = cube_of(p).astype(np.float64) * CUBE - 25.0
    return np.clip(np.floor((p64 - mn) * (1.0 / cell)).astype(np.int64), 0, nc - 1)


def gate_of(plane_res):
    return np.float32(3) * np.float32(plane_res)


_GG = 2.0 ** -12   # grid of every coordinate of a gate site but the tuned one
_EPS = 2.0 ** -11  # "within 1e-3 m" of a cell or cube face
GATE_DIRECTIONS = tuple((dx, dy, dz) for dx in (1, 0, -1) for dy in (1, 0, -1) for dz in (1, 0, -1) if (dx, dy, dz) != (0, 0, 0))
GATE_PLACEMENTS = ("cell_middle", "cell_face", "cell_corner", "cube_face")


def _ordered(x):
    """float32 -> integers in the order of the floats (one step = the adjacent float)"""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def _unordered(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(np.float32)


def _sphere(n):
    """n fixed unit vectors spread over the sphere"""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = i * np.pi * (3 - np.sqrt(5.0))
    return np.c_[np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z]


def gate_edge(plane_res):
    """A site: one query q, four map points at 0.8 r (r^2 = gate = float32(3) * float32(planeRes)) and a fifth ON the gate, along one
    of the 26 axis / face-diagonal / space-diagonal directions.  The fifth is tuned in ONE coordinate (axis t: the first the direction
    moves along), float by float: the `in` site of a pair holds the last configuration with d2_ref <= gate -- d2_ref == gate wherever a
    small change of the fifth's offset along another axis reaches it (`n_equal` sites) --, the `out` site the float-adjacent one with
    d2_ref > gate.  The two sites of a pair are the same configuration `shift` metres apart along axis s = t + 1: a whole number of
    cells that is exact on the 2^-12 grid all s coordinates lie on, so the pair differs by that one float and by nothing else.  Every
    other out site holds a sixth point at 1.3 r.
    Four placements of the query per direction: the middle of a cell; 2^-11 m inside the cell face the direction (axis t) points at (the
    fifth lies in the far part of the next cell); at the cell corner the direction points at (the fifth in the cell diagonally
    opposite, for a space diagonal the corner cell of the 27-cell block); 2^-11 m inside a cube face (axis f = t + 2) with the fifth
    inside the cube.  Axis t coordinates stay within 8 m of the origin (a float step there moves d2 by a few of its ulps); the sites
    spread along s and f, 6 m apart; the three groups t = x, y, z lie in different cubes.
    `patch`, `scan_a`, `pose_a`: a second registration far away for the binned-ahead path (see xruns)."""
    from fractions import Fraction
    f32, f64 = np.float32, np.float64
    gate = gate_of(plane_res)
    r = np.sqrt(f64(gate))
    nc, cell = grid_cells(plane_res)
    k = next(k for k in range(1, 200) if Fraction(50 * k, nc) >= 6 and (Fraction(50 * k, nc) / Fraction(1, 4096)).denominator == 1)
    shift = float(Fraction(50 * k, nc))
    snap = lambda v: np.round(np.asarray(v, f64) / _GG) * _GG
    sphere = _sphere(96)
    used = set()
    group_off = {0: np.zeros(3), 1: np.array([100.0, 0.0, 0.0]), 2: np.array([0.0, -100.0, 0.0])}  # (axis f of the group: two cubes away)
    rows = {}  # (group t, a row at a cube face?, its low face?) -> pairs handed out; a row holds per_row pairs along s
    per_row = int((92.0 - shift) // (2 * shift)) + 1
    regular = [(xt, xf) for xt in (-6.0, 0.0, 6.0) for xf in (-18.0, -12.0, -6.0, 0.0, 6.0, 12.0, 18.0)]
    mp, qs, sites = [], [], []
    n_equal = 0

    def tune(q, p, t, f, sg):
        """the float-adjacent pair of p[t] around the gate, moving away from q; the jitter of p[f] that reaches d2 == gate first"""
        best = None
        for j in range(96):
            pj = p.copy()
            pj[f] = p[f] + j * 2.0 ** -14
            rest = sum(f64(f32(f32(q[a]) - f32(pj[a]))) ** 2 for a in range(3) if a != t)
            o0 = _ordered(f32(q[t] + sg * np.sqrt(f64(gate) - rest)))
            cand = np.repeat(pj.astype(f32)[None], 129, 0)
            cand[:, t] = _unordered(o0 + sg * np.arange(-64, 65))
            dd = d2_ref(q.astype(f32), cand)
            assert (np.diff(dd) >= 0).all() and dd[0] <= gate < dd[-1]
            i = int(np.nonzero(dd <= gate)[0][-1])
            if best is None or dd[i] == gate:
                best = (cand[i].copy(), cand[i + 1].copy(), bool(dd[i] == gate))
            if dd[i] == gate:
                break
        return best

    for pair, (d, placement) in enumerate((d, pl) for d in GATE_DIRECTIONS for pl in GATE_PLACEMENTS):
        d = np.array(d)
        t = int(np.nonzero(d)[0][0]); s = (t + 1) % 3; f = (t + 2) % 3
        sg = int(d[t])
        cube_face = placement == "cube_face"
        low_face = d[f] >= 0
        kind = (t, cube_face, low_face and cube_face)
        n_in_kind = rows.get(kind, 0)
        rows[kind] = n_in_kind + 1
        row, m = divmod(n_in_kind, per_row)
        nominal = np.zeros(3)
        if cube_face:
            nominal[t] = (-6.0, 0.0, 6.0)[row]
        else:
            nominal[t], nominal[f] = regular[row]
        nominal[s] = -71.0 + m * 2 * shift
        kk = np.floor((nominal + 25.0) / cell)
        lo, hi = -25.0 + kk * cell, -25.0 + (kk + 1) * cell
        q = snap(0.5 * (lo + hi))
        toward = lambda a: snap(hi[a] - _EPS) if d[a] > 0 else snap(lo[a] + _EPS)  # (an axis the direction does not move along: the low side)
        if placement == "cell_face":
            q[t] = toward(t)
        if placement == "cell_corner":
            q = np.array([toward(a) for a in range(3)])
        if cube_face:
            q[f] = -25.0 + _EPS if low_face else 25.0 - _EPS
        q = q + group_off[t]
        assert np.array_equal(q.astype(f32).astype(f64), q)
        p = q + snap(r * d / np.linalg.norm(d))
        p_in, p_out, equal = tune(q, p, t, f, sg)
        n_equal += equal
        assert (cube_of(p_in) == cube_of(q)).all() and (cube_of(p_out) == cube_of(q)).all(), (plane_res, pair, "the fifth lies in the query's cube")
        sh = np.zeros(3); sh[s] = shift
        cfg_in = [q.astype(f32), p_in]
        cfg_out = [(q + sh).astype(f32), (p_out.astype(f64) + sh).astype(f32)]
        assert np.array_equal(cfg_out[1].astype(f64), p_out.astype(f64) + sh), "the shift is exact"

        def free(c):
            """c (at the in site) and its copy at the out site: on the grid, in the query's cube, in leaves nobody holds"""
            both = np.stack([c, c + sh])
            if not np.array_equal(both.astype(f32).astype(f64), both):
                return None
            if not ((cube_of(both[0]) == cube_of(q)).all() and (cube_of(both[1]) == cube_of(q + sh)).all()):
                return None
            leaves = [tuple(l) for l in _leaf(both, plane_res)]
            return None if (leaves[0] in used or leaves[1] in used or leaves[0] == leaves[1]) else leaves

        for l in _leaf(np.stack([p_in, p_out, cfg_out[1], (p_in.astype(f64) + sh).astype(f32)]), plane_res):
            used.add(tuple(l))
        near = []
        for u in sphere[np.argsort(-(sphere @ d), kind="stable")]:  # (nearest to the direction first: inside the cube at a cube face)
            c = q + snap(0.8 * r * u)
            leaves = free(c)
            if leaves is None or not (d2_ref(q.astype(f32), c.astype(f32)[None])[0] < 0.75 * gate):
                continue
            used.update(leaves); near.append(c)
            if len(near) == 4:
                break
        assert len(near) == 4, (plane_res, pair, "four nearer points")
        sixth = None
        if pair % 2 == 0:
            for u in sphere[np.argsort(sphere @ d, kind="stable")]:
                c = q + snap(1.3 * r * u)
                leaves = free(c)
                if leaves is not None:
                    used.update(leaves); sixth = c
                    break
            assert sixth is not None
        dname = "".join(("-", "0", "+")[v + 1] for v in d)
        for side, (qq, p5), off in (("in", cfg_in, np.zeros(3)), ("out", cfg_out, sh)):
            pts = [(c + off).astype(f32) for c in near] + [p5] + ([(sixth + off).astype(f32)] if side == "out" and sixth is not None else [])
            sites.append(dict(name=f"{dname}/{placement}/{side}", direction=tuple(d), placement=placement, side=side, query=len(qs),
                              first_point=sum(map(len, mp)), fifth=sum(map(len, mp)) + 4, n_points=len(pts), equal=bool(equal and side == "in"),
                              tuned_axis=t, shift_axis=s, sixth=len(pts) == 6))
            mp.append(np.array(pts, f32)); qs.append(qq)
    pitch = plane_res
    patch = _grid(_centres(-3 * pitch, 3 * pitch, pitch), _centres(150.0 - 3 * pitch, 150.0 + 3 * pitch, pitch), _centres(50.0 - 3 * pitch, 50.0 + 3 * pitch, pitch))
    mp.append(patch.astype(f32))
    g = np.arange(-20.0, 20.0, 0.8)
    scan_a = _grid(g, g, np.array([-50.8, -50.0, -49.2])).astype(f32)
    return Family(f"gate_edge_{plane_res}", np.concatenate(mp), np.array(qs, f32), plane_res, sites=sites, n_equal=n_equal, shift=shift,
                  gate=gate, scan_a=scan_a, pose_a=XRUNS_POSE_A, aim="gate")


# ------------------------------------------------------------------------------------------------------------------------
# 7. interior cell faces of grids whose cell is no binary fraction (57 cells at planeRes 0.25, 45 at 0.4)
# ------------------------------------------------------------------------------------------------------------------------
def _around(face_exact):
    """the largest float below an exact (rational) coordinate and the smallest at or above it"""
    from fractions import Fraction
    v = np.float32(float(face_exact))
    if Fraction(float(v)) >= face_exact:
        return np.nextafter(v, np.float32(-np.inf)), v
    return v, np.nextafter(v, np.float32(np.inf))


def cell_faces(plane_res, seed=8):
    """Cube (0, 0, 0); cell faces -25 + k * (50 / nc) for k = 1, nc // 2 and nc - 1.  A site lies on one face (each axis), on an edge
    (two faces) or at a corner (three) of a cell, its queries on ONE side of every face of the site: at the nearest float at or above
    the face and 1e-4 m above it (high), or at the nearest float below it and 1e-4 m below it (low).  Around the site a lattice of leaf
    centres (pitch = planeRes), with a hole of 2.25 pitches on the queries' side, and -- per face -- four map points ON it, at those
    same four coordinates, each in a leaf of its own next to the site's centre: the nearest neighbours of a query lie at and across
    the cell face, in the cell the fp64 expression of the product puts them in.  `info`: the cell of every map point and query
    (cell_of), the sites, and per face its exact position."""
    from fractions import Fraction
    f32 = np.float32
    nc, cell = grid_cells(plane_res)
    pitch = plane_res
    specials, lattices, qs, holes, sites, face_values = [], [], [], [], [], {}
    n = 0
    for k in (1, nc // 2, nc - 1):
        exact = Fraction(-25) + k * Fraction(50, nc)
        below, at = _around(exact)
        face_values[k] = (exact, below, at)
        four = [below, at, f32(float(exact) - 1e-4), f32(float(exact) + 1e-4)]
        for i, axes in enumerate(((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))):
            for high in (True, False):
                u = -22.0 + 3.4 * (2 * i + high) + 0.37
                c = np.array([float(exact) if a in axes else u for a in range(3)])
                cent = [_centres(c[a] - 4 * pitch, c[a] + 4 * pitch, pitch) for a in range(3)]
                mid = [int(np.searchsorted(cent[a], c[a])) for a in range(3)]
                lattices.append(_grid(*cent).astype(f32))
                holes.append((axes, high, at, c))
                for a in (axes if high or len(axes) < 3 else ()):  # (a corner's two sites share their centre and these points)
                    b, e = (a + 1) % 3, (a + 2) % 3
                    for j, v in enumerate(four):
                        p = np.zeros(3, f32)
                        p[a], p[b], p[e] = v, cent[b][mid[b] + j - 2], cent[e][mid[e] - 1 + a]
                        specials.append(p)
                vals = [([at, four[3]] if high else [below, four[2]]) if a in axes else [f32(c[a] + o * pitch) for o in (0.0, 0.5, -1.15)] for a in range(3)]
                q = _grid(*vals).astype(f32)
                sites.append(dict(k=k, axes=axes, high=high, first_query=n, n_queries=len(q)))
                n += len(q)
                qs.append(q)
    lat = np.concatenate(lattices)
    lat = lat[(cube_of(lat) == 0).all(1)]
    for axes, high, at, c in holes:
        own = np.all([(lat[:, a] >= at) == high for a in axes], axis=0)
        lat = lat[~(own & (np.abs(lat.astype(np.float64) - c).max(1) < 2.25 * pitch))]
    specials = _first_per_leaf(np.array(specials, f32), plane_res)  # (where two sites meet, the first one's point holds the leaf)
    mp = _first_per_leaf(np.concatenate([specials, lat]), plane_res)
    assert np.array_equal(mp[:len(specials)], specials)
    for k, (exact, below, at) in face_values.items():
        for a in range(3):
            assert (specials[:, a] == below).any() and (specials[:, a] == at).any(), "map points float-adjacent across every face, on every axis"
    q = np.concatenate(qs)
    return Family(f"cell_faces_{plane_res}", mp, q, plane_res, n_on_faces=len(specials), sites=sites, face_values=face_values,
                  map_cells=cell_of(mp, plane_res), query_cells=cell_of(q, plane_res), aim="cells")


# ------------------------------------------------------------------------------------------------------------------------
# 8. scan rows that are not finite, or far outside any window
# ------------------------------------------------------------------------------------------------------------------------
def nonfinite_rows(scan):
    """A copy of the scan with NaN, +inf, -inf and 1e12 in single coordinates (every value on every axis) of its first and last row, of
    rows 63 and 64, of a run of 64 consecutive rows and of a run of 16; and the sorted list of those rows."""
    out = np.array(scan, np.float32, copy=True)
    n = len(out)
    assert n >= 1024
    rows = np.array([0, 63, 64] + list(range(n // 4 + 3, n // 4 + 67)) + list(range(n // 2 + 5, n // 2 + 21)) + [n - 1])
    assert len(np.unique(rows)) == len(rows) == 84 and (np.diff(rows) > 0).all()
    bad = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(1e12))
    for j, row in enumerate(rows):
        out[row, j % 3] = bad[j % 4]
    return out, rows


GATE_RES = (0.2, 0.33, 0.4, 0.8)
CELL_FACE_RES = (0.25, 0.4)
NEW_FAMILIES = tuple(f"gate_edge_{r}" for r in GATE_RES) + tuple(f"cell_faces_{r}" for r in CELL_FACE_RES) + ("faces_0.4", "faces_0.8")

FAMILIES = {
    "ties_volume_0.25": lambda: ties_volume(0.25),
    "ties_volume_0.125": lambda: ties_volume(0.125),
    "ties_volume_0.2": lambda: ties_volume(0.2),
    "ties_sheets_0.25": lambda: ties_sheets(0.25),
    "ties_sheets_0.2": lambda: ties_sheets(0.2),
    "near_ties": near_ties,
    "dense": dense,
    "faces": faces,
    "xruns": xruns,
    **{f"gate_edge_{r}": (lambda r=r: gate_edge(r)) for r in GATE_RES},
    **{f"cell_faces_{r}": (lambda r=r: cell_faces(r)) for r in CELL_FACE_RES},
    "faces_0.4": lambda: faces(0.4),
    "faces_0.8": lambda: faces(0.8),
}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]
