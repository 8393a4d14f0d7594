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
              face; cubes of 4, 5 and 6 points; the last cube of the 21 x 21 x 11 window and a query beyond it
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
def faces(seed=5):
    """planeRes 0.2.  A site sits at a point c of a cube face, edge or corner: a lattice of 2 m around c, thinned out INSIDE the
    queries' own cube to the points at least 0.45 m (Chebyshev) from c, so that the points across the face are the nearest ones.  The
    queries lie in one cube per site: the high side (on the face itself, one ulp, 1e-4 and 1e-3 beyond it) or the low side."""
    rng = np.random.default_rng(seed)
    plane_res, pitch = 0.2, 0.2
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
    seen = {}
    for axes, c in site_list:
        key = tuple(c)
        assert key not in seen, "every site has a lattice of its own"
        g = _grid(_centres(c[0] - 1.0, c[0] + 1.0, pitch), _centres(c[1] - 1.0, c[1] + 1.0, pitch), _centres(c[2] - 1.0, c[2] + 1.0, pitch)).astype(np.float32)
        vals = [None, None, None]
        for a in range(3):
            if a in axes:
                vals[a] = side_values(*axes[a])
            else:
                vals[a] = [f32(c[a] + d) for d in (0.0, 0.1, -0.23) + tuple(rng.uniform(-0.3, 0.3, 1))]
        q = _grid(*vals).astype(np.float32)
        qcube = cube_of(q)
        assert (qcube == qcube[0]).all()
        own = (cube_of(g) == qcube[0]).all(1)
        near = np.abs(g.astype(np.float64) - c).max(1) < 0.45
        seen[key] = g[~(own & near)]
        qs.append(q)
    mp += list(seen.values())
    # cubes holding exactly 4, 5 and 6 points
    for n, cx in ((4, 150.0), (5, 200.0), (6, 250.0)):
        pts = np.array([cx, 10.0, 0.0]) + (np.arange(n)[:, None] * np.array([0.25, 0.0, 0.0]) + np.array([[0, 0.3 * (i % 2), 0.3 * (i % 3)] for i in range(n)]))
        mp.append(pts.astype(np.float32))
        qs.append((pts[:3] + np.array([0.05, 0.02, -0.04])).astype(np.float32))
        qs.append(np.array([[cx + 0.6, 10.1, 0.2], [cx - 3.0, 9.0, 0.0]], np.float32))
    # the last cube of the window in x (cubes -10 .. 10 around a sensor at the origin: x in [-525, 525)) and beyond it
    edge = _grid(_centres(523.0, 525.0, pitch), _centres(-1.0, 1.0, pitch), _centres(-1.0, 1.0, pitch)).astype(np.float32)
    edge = edge[edge[:, 0] < f32(524.95)]
    mp.append(edge)
    eq = _grid([f32(524.0), f32(524.9), np.nextafter(f32(525.0), f32(-np.inf)), f32(525.0), f32(525.5), f32(-526.0)], [f32(0.0), f32(0.31)], [f32(0.1), f32(-0.45)])
    qs.append(eq.astype(np.float32))
    # first and last cell of a cube, away from any site: the clamped neighbourhood over an ordinary lattice
    for cx in (-24.9, 24.9):
        g = _grid(_centres(cx - 1.0 if cx > 0 else -25.0, 25.0 if cx > 0 else cx + 1.0, pitch), _centres(-20.0, -18.0, pitch), _centres(3.0, 5.0, pitch))
        mp.append(g.astype(np.float32))
        qs.append((np.array([cx, -19.0, 4.0]) + rng.uniform(-0.08, 0.08, (40, 3))).astype(np.float32))
    n_face = sum(len(q) for q in qs[:len(site_list)])
    return Family("faces", np.concatenate(mp), np.concatenate(qs), plane_res, n_face_queries=n_face, aim="faces")


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
}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]
