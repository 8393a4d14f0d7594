"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np

from superodom_amd import synth


def build_oracle_map_from(oracle, points, plane_res, origin_t, raw=True):
    m = oracle.OracleMap(plane_res=plane_res)
    m.set_origin(np.asarray(origin_t, float))
    m.add_surf(points, raw=raw)
    return m


def pose_close(a, b, tol_t=1e-4, tol_r=1e-4):
    dt, dr = synth.pose_error(a, b)
    return dt <= tol_t and dr <= tol_r, dt, dr


TOL_T, TOL_R = 1e-4, 1e-4  # north_star: <=1e-4 m translation / <=1e-4 rad rotation

# ------------------------------------------------------------------------------------------------------------------------
# "The same registration": ONE definition for product against product (to the bit) and one for product against oracle.
# ------------------------------------------------------------------------------------------------------------------------
ITER_FIELDS = ("lm_iterations", "num_successful_steps", "termination", "num_surf_from_scan", "reject_hist", "obs_hist",
               "initial_cost", "final_cost", "pose_after", "translation_norm", "rotation_norm")
STATS_FIELDS = ("JtJ", "Jtr", "uncertainty", "pos_in_localmap", "laser_cloud_surf_from_map_num", "laser_cloud_corner_from_map_num",
                "laser_cloud_surf_stack_num", "laser_cloud_corner_stack_num", "startup_count",
                "total_translation", "total_rotation", "translation_from_last", "rotation_from_last")
# What is a floating-point sum over the residuals, or follows from one: its bits follow the summation tree.  Runs that change the tree
# (map or queries sharded over ranks) hold these to a tolerance of their own and pass this as omit=.
SUMMED_FIELDS = ("initial_cost", "final_cost", "pose_after", "translation_norm", "rotation_norm", "JtJ", "Jtr",
                 "total_translation", "total_rotation", "translation_from_last", "rotation_from_last")
# What the context carries over from the call before (so_icp_ctx::prev_obs_hist, ::startup_count): equal only after equal call histories.
CARRIED_OVER_FIELDS = ("uncertainty", "startup_count")


def _bits(v):
    if isinstance(v, int):
        return v
    if isinstance(v, float):
        return np.float64(v).tobytes()
    a = np.ctypeslib.as_array(v)
    return tuple(a.tolist()) if a.dtype.kind in "iu" else a.tobytes()


def stats_bits(st, *, omit=()):
    """Every deterministic field of a product Stats as a tuple of (field, outer iteration or None, value) -- hashable, picklable,
    floats by their bytes: n_iterations, per outer iteration ITER_FIELDS, then STATS_FIELDS.

    Not in the set, because they describe the path taken and not the registration: time_elapsed_ms (wall clock), flags (which host
    schedule ran: staged, binned ahead, chained, per-evaluation launches ...) and prediction_source (always written 0,
    icp_context.cpp fill_result).  total_* and *_from_last ARE in the set: fill_result computes them from the guess and the final
    pose of this call alone, not from earlier calls.  uncertainty and startup_count are in the set too, but come from the call
    before (CARRIED_OVER_FIELDS): a site that compares contexts with different call histories omits them.  The reserved words and
    num_corner_from_scan (never written: no edge features) are left out."""
    unknown = set(omit) - set(ITER_FIELDS) - set(STATS_FIELDS)
    assert not unknown, f"omit= names no field of the set: {sorted(unknown)}"
    out = [("n_iterations", None, st.n_iterations)]
    for it in range(st.n_iterations):
        out += [(f, it, _bits(getattr(st.iterations[it], f))) for f in ITER_FIELDS if f not in omit]
    out += [(f, None, _bits(getattr(st, f))) for f in STATS_FIELDS if f not in omit]
    return tuple(out)


def stats_of(res):
    """(rc, pose, Stats) of a registration -> (rc, pose as a list, flags, stats_bits): the form a rank process sends to its parent"""
    rc, pose, st = res
    return rc, np.asarray(pose).tolist(), st.flags, stats_bits(st)


def bits_field(bits, name, it=None):
    """one field out of a stats_bits() value (floats as their bytes)"""
    return next(v for f, i, v in bits if f == name and i == it)


def assert_same_bits(a, b, tag, *, omit=()):
    """Two product registrations are the same one, bit for bit.  a, b: Stats, or stats_bits() of one (what a worker process sends)."""
    assert set(omit) <= set(ITER_FIELDS) | set(STATS_FIELDS), f"omit= names no field of the set: {sorted(set(omit) - set(ITER_FIELDS) - set(STATS_FIELDS))}"
    a, b = [x if isinstance(x, tuple) else stats_bits(x) for x in (a, b)]
    a, b = [tuple(e for e in x if e[0] not in omit) for x in (a, b)]
    if a == b:
        return
    assert a[0] == b[0], f"{tag}: n_iterations differs: {a[0][2]} != {b[0][2]}"
    diff = [(x[0], x[1]) for x, y in zip(a, b) if x != y]
    f, it = diff[0]
    x, y = [next(e[2] for e in s if e[:2] == (f, it)) for s in (a, b)]
    x, y = [np.frombuffer(v, np.float64).tolist() if isinstance(v, bytes) else v for v in (x, y)]
    where = "" if it is None else f" at iteration {it}"
    raise AssertionError(f"{tag}: {f} differs{where}: {x} != {y} (every differing field: {diff})")


def assert_rank_follows_single(a, ref, tag, *, omit=()):
    """a, ref: stats_of() of one rank of a sharded run and of the single context.  The ranks add their partial sums in another order
    than one context adds the whole: the float fields are held to 1e-9 through the pose ("changes the summation tree, not the
    tolerance"), everything else to the bit."""
    assert a[0] == ref[0] == 0, (tag, a[0], ref[0])
    assert_same_bits(a[3], ref[3], tag, omit=SUMMED_FIELDS + tuple(omit))
    ok, dt, dr = pose_close(np.array(a[1]), np.array(ref[1]), 1e-9, 1e-9)
    assert ok, (tag, dt, dr)


def assert_follows_oracle(st, ost, tag, *, pose=None, opose=None, omit=(), cost_rtol=1e-9, pose_tol=1e-8):
    """A product Stats (or a second oracle Stats) against the oracle's for the same scan, guess and map: outer iteration count first, then per outer iteration
    the LM iteration count, accepted steps, termination code, matched points, both histograms and the final cost (relative); with
    the poses given, the tolerance of record and then near-machine agreement."""
    known = ("lm_iterations", "num_successful_steps", "termination", "num_surf", "reject_hist", "obs_hist", "final_cost")
    assert set(omit) <= set(known), f"omit= names no field of the set: {sorted(set(omit) - set(known))}"
    assert st.n_iterations == ost.n_iterations, f"{tag}: n_iterations differs: {st.n_iterations} != {ost.n_iterations} (outer iteration counts must agree before anything else is compared)"
    bad = []
    for it in range(st.n_iterations):
        a, b = (st.iterations if hasattr(st, "iterations") else st.iters)[it], ost.iters[it]
        for f in known[:-1]:
            x, y = getattr(a, "num_surf_from_scan" if f == "num_surf" and hasattr(a, "num_surf_from_scan") else f), getattr(b, f)
            x, y = (x, y) if isinstance(x, int) else (list(x), list(y))
            if f not in omit and x != y:
                bad.append((f, it, x, y))
        if "final_cost" not in omit and not abs(a.final_cost - b.final_cost) <= cost_rtol * max(1.0, abs(b.final_cost)):
            bad.append(("final_cost", it, a.final_cost, b.final_cost))
    if bad:
        f, it, x, y = bad[0]
        raise AssertionError(f"{tag}: {f} differs at iteration {it}: {x} != {y} (every differing field: {[e[:2] for e in bad]})")
    if pose is not None:
        ok, dt, dr = pose_close(pose, opose, TOL_T, TOL_R)
        assert ok, f"{tag}: pose parity violated: dt={dt:.3e} m dr={dr:.3e} rad"
        assert dt < pose_tol and dr < pose_tol, f"{tag}: expected near machine agreement, got {dt:.3e} {dr:.3e}"


# ------------------------------------------------------------------------------------------------------------------------
# Set-up shared by the parity tests.
# ------------------------------------------------------------------------------------------------------------------------
def scene_with_oracle(scene, oracle, make, *, oracle_too=True, **cfg):
    """(scene, product context holding the scene's map, oracle map filled from the context's export_map() -- the canonical order, so
    that the tie-break "earlier index first" is shared).  scene: a synth.Scene name or a scene object."""
    sc = synth.Scene(scene) if isinstance(scene, str) else scene
    oracle_res = {k: cfg[k] for k in ("plane_res", "line_res") if k in cfg} or dict(plane_res=sc.plane_res)  # (the oracle's own default line_res otherwise)
    for k, v in dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1).items():
        cfg.setdefault(k, v)
    slam = make(**cfg)
    # default window (origin_ = (10,10,5), LocalMap.h:141-144): world cube 0 sits in the middle of the block array.
    # (LocalMap::setOrigin puts the sensor's cube at index 0, which drops every negative-side cube until the
    #  first shiftMap -- exercised in test_localization_sequence_with_map_updates.)
    n = slam.add_surf_point_cloud(sc.map_points)
    assert n == len(sc.map_points) == slam.map_size()
    if not oracle_too:
        return sc, slam, None
    exported = slam.export_map()
    assert len(exported) == slam.map_size()
    om = oracle.OracleMap(**oracle_res)
    assert om.add_surf(exported, raw=True) == len(exported)
    return sc, slam, om


def chain_deltas(sc, ids, *, off=None, x_off=None):
    """Motion predictions that put guess k near sc.guess(ids[k]): gt(k-1)^-1 o guess(k) (the registration of k - 1 ends within
    millimetres of gt).  off = {k: (dt, dth_deg)}: scan k starts that far from its ground truth instead.  x_off = {k: metres}: the
    prediction of frame k is that far off along x."""
    d = np.zeros((len(ids), 7)); d[:, 6] = 1.0
    for k in range(1, len(ids)):
        g = sc.guess(ids[k]) if off is None or k not in off else synth.perturb_pose(sc.gt_pose(ids[k]), 77 + k, *off[k])
        d[k] = synth.pose_between(sc.gt_pose(ids[k - 1]), g)
        if x_off and k in x_off:
            d[k, 0] += x_off[k]
    return d


def run_staged_stream(slam, scans, guesses, order, step=None):
    """The bench / node pattern: announce the next scan, register the current one.  step(k, i) replaces the plain
    slam.register(scans[i], guesses[i]) of position k in the order."""
    res = []
    slam.stage_scan(scans[order[0]])
    for k, i in enumerate(order):
        if k + 1 < len(order):
            slam.stage_scan(scans[order[k + 1]])
        res.append(slam.register(scans[i], guesses[i]) if step is None else step(k, i))
    return res


def noisy_planes_cloud(n, rng, offset=(0.0, 0.0, 0.0), sigma=0.01):
    """Four noisy planes (floor/ceiling/2 walls) inside one 50 m cube -- the SURVEY App. D probe scene."""
    k = n // 4
    parts = []
    xy = rng.random((k, 2)) * 40 - 20
    parts.append(np.c_[xy, -1.5 + sigma * rng.standard_normal(k)])
    xy = rng.random((k, 2)) * 40 - 20
    parts.append(np.c_[xy, 6.0 + sigma * rng.standard_normal(k)])
    xz = np.c_[rng.random(k) * 40 - 20, rng.random(k) * 7.5 - 1.5]
    parts.append(np.c_[xz[:, 0], 10.0 + sigma * rng.standard_normal(k), xz[:, 1]])
    yz = np.c_[rng.random(n - 3 * k) * 40 - 20, rng.random(n - 3 * k) * 7.5 - 1.5]
    parts.append(np.c_[-12.0 + sigma * rng.standard_normal(n - 3 * k), yz[:, 0], yz[:, 1]])
    return (np.concatenate(parts) + np.asarray(offset)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# A scene on which the reference's OWN k-NN engine (flann/octree.h, compiled into oracle/_ref) is exact, so that a whole
# registration can be run with it in the loop and compared with the exact-search oracle and the product.
#
# The stock octree has two defects: initialize() derives the y / z bounds of the root cube from comparisons
# against x (oct.h:384-385), and inside() tests the query's X coordinate against all three octant centres (oct.h:988-990).
# Both are inert when, in every 50 m block, (a) the points' x range is at least as large as their y and z ranges -- the root
# cube, sized by the x range, then contains every point wherever the broken y / z centres land -- and (b) x is far from every
# y and z coordinate of the block -- inside() then never answers "yes" early and the search degenerates to an exhaustive,
# correctly pruned one.  A corridor along x at x ~ 1 100 m (y within +-6.5 m, z within -1.5 .. 4.1 m) has both properties.
# ------------------------------------------------------------------------------------------------------------------------
class CorridorScene:
    X0, LEN = 1003.7, 170.0

    def __init__(self, plane_res=0.2, rings=32, azimuth=512, fov_deg=22.5, seed=21):
        rng = np.random.default_rng(seed)
        R = []

        def add(o, u, v):
            R.append((np.array(o, float), np.array(u, float), np.array(v, float)))
        x0, L, z0, z1, ya, yb = self.X0, self.LEN, -1.5, 4.1, -6.3, 5.9
        H = z1 - z0
        add([x0, ya, z0], [L, 0, 0], [0, yb - ya, 0])          # floor
        add([x0, ya, z1], [L, 0, 0], [0, yb - ya, 0])          # ceiling
        add([x0, ya, z0], [L, 0, 0], [0, 0, H])                # side walls
        add([x0, yb, z0], [L, 0, 0], [0, 0, H])
        add([x0, ya, z0], [0, yb - ya, 0], [0, 0, H])          # end walls
        add([x0 + L, ya, z0], [0, yb - ya, 0], [0, 0, H])
        k = 0
        for xc in np.arange(x0 + 11.6, x0 + L - 5.0, 12.3):    # partial cross walls, alternating sides: they fix the pose along x
            if k % 2 == 0:
                add([xc, ya, z0], [0, 4.6 + rng.random(), 0], [0, 0, H])
            else:
                add([xc, yb, z0], [0, -(4.3 + rng.random()), 0], [0, 0, H])
            k += 1
        for _ in range(14):                                     # leaning panels: roll / pitch observability
            cx = x0 + 4.0 + rng.random() * (L - 12.0); cy = ya + 0.8 + rng.random() * (yb - ya - 4.5)
            Lp, Wp = 1.5 + 1.5 * rng.random(), 1.5 + 1.5 * rng.random()
            if rng.random() < 0.5:
                add([cx, cy, z0], [Lp, 0, Lp], [0, Wp, 0])
            else:
                add([cx, cy, z0], [0, Lp, Lp], [Wp, 0, 0])
        w = synth.World.__new__(synth.World)
        w.o = np.stack([r[0] for r in R]); w.u = np.stack([r[1] for r in R]); w.v = np.stack([r[2] for r in R])
        n = np.cross(w.u, w.v)
        w.n = n / np.linalg.norm(n, axis=1, keepdims=True)
        w.extent = L
        w._groups = None
        self.world = w
        self.plane_res = plane_res
        self.map_points = synth.sample_map(w, plane_res, None, seed=seed + 1)
        self.dirs = synth.lidar_dirs(rings, azimuth, fov_deg)

    def gt_pose(self, i):
        s = i / 7.0
        t = np.array([self.X0 + 62.0 + 9.0 * s, -0.9 + 1.1 * np.sin(2.0 * s), 0.15 * np.cos(3.0 * s)])
        q = synth.quat_from_rotvec(np.array([0.02 * np.sin(5 * s), 0.03 * np.cos(3 * s), 0.2 + 0.7 * s]))
        return np.concatenate([t, q])

    def scan(self, i):
        return synth.raycast(self.world, self.gt_pose(i), self.dirs, seed=40 + i)

    def guess(self, i, dt=0.10, dth_deg=1.0):
        return synth.perturb_pose(self.gt_pose(i), 2000 + i, dt, dth_deg)


# ------------------------------------------------------------------------------------------------------------------------
# Rank-deficient geometry (VERDICT r04 "weak" 1 / "next" 6b): scenes whose normal equations J^T J are ill conditioned because part
# of the pose is not observable.  The product solves the LM step by Cholesky on the scaled normal equations (lm_solver.h), the
# oracle by QR on the stacked Jacobian like Ceres DENSE_QR: normal equations square the condition number, so this is where the
# two could part.  sigma = noise of map and scan along the normals (LidarSlam.cpp:772 rejects noise-free planes).
# ------------------------------------------------------------------------------------------------------------------------
DEGENERATE_RECTS = {
    # one plane: x, y and yaw are unobservable (they move only through the 1 cm noise of the normals)
    "floor_only": [([-20, -20, -1.5], [40, 0, 0], [0, 40, 0])],
    # corridor along x without end or cross walls: the translation along x is unobservable
    "open_corridor": [([-24, -6.3, -1.5], [48, 0, 0], [0, 12.2, 0]), ([-24, -6.3, 4.1], [48, 0, 0], [0, 12.2, 0]),
                      ([-24, -6.3, -1.5], [48, 0, 0], [0, 0, 5.6]), ([-24, 5.9, -1.5], [48, 0, 0], [0, 0, 5.6])],
    # two parallel walls: only the translation along their normal and the two rotations that tilt them are observable
    "two_walls": [([-20, -6.3, -1.5], [40, 0, 0], [0, 0, 7.5]), ([-20, 5.9, -1.5], [40, 0, 0], [0, 0, 7.5])],
    # a room corner AT THE WORLD ORIGIN: floor z = 0 and the walls x = 0, y = 0 all contain the origin, where the reference's plane
    # parameterisation A x = -1 (LidarSlam.cpp:798-816) is ill conditioned (|x| = 1 / offset; only the 1 cm noise keeps it finite).
    # Well conditioned as a registration (three orthogonal planes): every pose component is observable.
    "origin_corner": [([0, 0, 0], [24, 0, 0], [0, 24, 0]), ([0, 0, 0], [0, 24, 0], [0, 0, 8]), ([0, 0, 0], [24, 0, 0], [0, 0, 8])],
}
# rows of the 6-vector [dt_x, dt_y, dt_z, rotvec_x, rotvec_y, rotvec_z] (world frame) the scene DOES constrain
DEGENERATE_OBSERVABLE = {"floor_only": [2, 3, 4], "open_corridor": [1, 2, 3, 4, 5], "two_walls": [1, 3, 5], "origin_corner": [0, 1, 2, 3, 4, 5]}
DEGENERATE_SENSOR_OFFSET = {"origin_corner": [5.3, 4.9, 1.8]}  # (the sensor stands inside the corner, 2 m above the floor)


class DegenerateScene:
    def __init__(self, name, plane_res=0.2, rings=32, azimuth=512, fov_deg=22.5, sigma=0.01):
        rects = DEGENERATE_RECTS[name]
        w = synth.World.__new__(synth.World)
        w.o = np.stack([np.array(r[0], float) for r in rects]); w.u = np.stack([np.array(r[1], float) for r in rects])
        w.v = np.stack([np.array(r[2], float) for r in rects])
        n = np.cross(w.u, w.v)
        w.n = n / np.linalg.norm(n, axis=1, keepdims=True)
        w.extent = 24.0
        w._groups = None
        self.name, self.world, self.plane_res, self.sigma = name, w, plane_res, sigma
        self.map_points = synth.sample_map(w, plane_res, None, seed=5, sigma=sigma)
        self.dirs = synth.lidar_dirs(rings, azimuth, fov_deg)
        self.observable = DEGENERATE_OBSERVABLE[name]

    def gt_pose(self, i):
        off = np.array(DEGENERATE_SENSOR_OFFSET.get(self.name, [0, 0, 0]), float)
        return np.concatenate([off + [0.7 + 0.5 * i, -0.9 + 0.3 * i, 0.2], synth.quat_from_rotvec(np.array([0.02, -0.03, 0.4 + 0.3 * i]))])

    def scan(self, i):
        return synth.raycast(self.world, self.gt_pose(i), self.dirs, seed=60 + i, sigma=self.sigma)

    def guess(self, i, dt=0.10, dth_deg=1.0):
        return synth.perturb_pose(self.gt_pose(i), 3000 + i, dt, dth_deg)


def pose_delta6(a, b):
    """[dt (world), rotation vector of qa^-1 qb rotated to the world frame] -- small-angle 6-vector between two poses"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    qa = a[3:] / np.linalg.norm(a[3:]); qb = b[3:] / np.linalg.norm(b[3:])
    dq = synth.quat_mul(np.array([-qa[0], -qa[1], -qa[2], qa[3]]), qb)
    if dq[3] < 0:
        dq = -dq
    rv = 2.0 * dq[:3]
    return np.concatenate([b[:3] - a[:3], synth.quat_to_R(qa) @ rv])


# Rank processes with the GPU open at the same time in the multi-process tests: with the pytest process itself, five.  Where
# there are more ranks than that on a device, the ranks of that device share processes.
MAX_RANK_PROCESSES = 4


def in_threads(n, fn, timeout=240):
    """fn(0) .. fn(n - 1), one thread each (ranks whose solve launches wait for each other must be driven at the same time)."""
    import threading
    out = [None] * n

    def run(r):
        out[r] = fn(r)
    th = [threading.Thread(target=run, args=(r,)) for r in range(n)]
    [t.start() for t in th]; [t.join(timeout) for t in th]
    assert all(o is not None for o in out), "a rank did not return"
    return out


def rank_groups(world, n_dev, max_procs=MAX_RANK_PROCESSES):
    """Ranks -> processes, rank r on device r % n_dev.  A process only ever holds ranks of ONE device: ranks of one process
    connect their peer inboxes by pointer, which is valid on the same device only.  At most max_procs processes where the
    device count allows it (one rank per device otherwise)."""
    n_used = min(world, n_dev)
    per_dev = max(1, max_procs // n_used)
    groups = []
    for d in range(n_used):
        ranks = list(range(d, world, n_dev))
        k = min(per_dev, len(ranks))
        groups += [ranks[i * len(ranks) // k:(i + 1) * len(ranks) // k] for i in range(k)]
    return groups


def by_rank(groups, per_process):
    """Per-process lists (in the order of `groups`) -> one list in rank order."""
    out = [None] * sum(len(g) for g in groups)
    for g, items in zip(groups, per_process):
        assert len(items) == len(g)
        for r, x in zip(g, items):
            out[r] = x
    return out
