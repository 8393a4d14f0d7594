"""-m gpu: the path-directed k-NN inputs (knn_edge_data.py; their properties are asserted on the CPU by test_knn_edges_host.py)
through every implementation of the exact 5-NN contract -- Seam B (knn_only_kernel + knn_fallback_kernel), the chunked sweep of a
registration with and without packed light chunks (knn_plane_kernel), its instrumented instantiation with the branch counters, the
one-wavefront-per-query sweep (knn_query_wave_kernel) and the batched sweep -- against the oracle (its map loaded from export_map(),
so the index orders coincide) and against the numpy reference.  EVERY query is compared and every comparison is exact: status
bytes, neighbour coordinates, canonical indices, bits of d2.  The gate sites (gate_edge: a fifth neighbour ON d2[4] == 3 * planeRes
and one float outside it, on four grids) are also checked by name; Seam B also for k = 1 .. 4; and a scan with NaN, +-inf and 1e12
in some of its rows goes through the chunked sweep, the query waves, a scan binned ahead, a resident scan and a batch."""
import numpy as np
import pytest

import knn_edge_data as ked
from helpers import CARRIED_OVER_FIELDS, assert_follows_oracle, assert_same_bits

pytestmark = pytest.mark.gpu

NAMES = list(ked.FAMILIES)
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])
JUDGED = (0, 3, 4, 5)  # five neighbours inside the gate: the fit pass judged the query, its neighbour list is the sweep's
ABLATE_STATS_ONLY = "65536"  # SOICP_ABLATE bit 16 (kernels.h): the instrumented instantiation with its statistics, nothing switched off


def _product(make, fam, **kw):
    cfg = dict(plane_res=fam.plane_res, line_res=fam.plane_res / 2, max_surface_features=-1, max_iterations=1)
    cfg.update(kw)
    slam = make(**cfg)
    slam.add_surf_point_cloud(fam.map_points)
    return slam


_setups = {}


def _setup(oracle, make, name):
    """family, export_map() of the product (canonical order), the oracle loaded from it, the numpy reference on it"""
    if name not in _setups:
        fam = ked.family(name)
        slam = _product(make, fam)
        exp = slam.export_map()
        slam.close()
        # the lattice survives the product's voxel filter: the map IS the generated one
        order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
        assert np.array_equal(order(exp).view(np.uint32), order(fam.map_points).view(np.uint32))
        om = oracle.OracleMap(plane_res=fam.plane_res)
        om.add_surf(exp, raw=True)
        assert np.array_equal(om.export(), exp), "oracle and product hold the map in the same order"
        scan = _scan_of(fam)
        ref = ked.brute_knn(exp, scan)
        _setups[name] = (fam, exp, om, scan, ref)
    return _setups[name]


def _scan_of(fam):
    """the family's queries as a scan of more than 4 096 points (the chunked sweep).  The filler is a line of points 1 mm apart at
    y = 40, z = 9, farther than the gate from every map point of every family (no cube there, or TOO_FAR) -- never a copy of a query
    of the family, whose chunks must keep the sizes they were made with."""
    q = fam.queries
    if len(q) > 4200:
        return q
    filler = np.array([[3.0, 40.0, 9.0]], np.float32) + np.arange(4200 - len(q), dtype=np.float32)[:, None] * np.array([[0.001, 0, 0]], np.float32)
    return np.ascontiguousarray(np.concatenate([q, filler]), np.float32)


def _expect_status(fam, ref):
    found, idx, d2, nbr = ref
    gate = np.float64(np.float32(3) * np.float32(fam.plane_res))
    st = np.where(~found, 1, np.where(d2[:, 4].astype(np.float64) > gate, 2, 0))
    return st


def _check_gate_sites(fam, ms, what):
    """gate_edge under the identity: TOO_FAR on exactly the `out` sites, a judged status on exactly the `in` ones -- by site name"""
    if fam.info["aim"] != "gate":
        return
    sites = fam.info["sites"]
    not_far = [s["name"] for s in sites if s["side"] == "out" and ms[s["query"]] != 2]
    not_judged = [s["name"] for s in sites if s["side"] == "in" and ms[s["query"]] not in JUDGED]
    assert not not_far and not not_judged, (what, "out sites not TOO_FAR", not_far, "in sites not judged", not_judged,
                                            "of them with d2[4] == gate exactly", [s["name"] for s in sites if s["equal"] and s["name"] in not_judged])


CAP_PER_SLOT = 1 << 20  # a canonical index of the device map is (slot of the cube) * 2^20 + position inside the cube (device_map.h)


def _export_index(exp, nb, cube):
    """canonical indices [n, 5] -> rows of export_map(), which walks the cubes in window order and each cube by ascending position.
    Which slot holds which cube is learnt from the lists themselves (cube [n, 3]: the cube each list must lie in) and must be one
    consistent assignment; that the rows are the right ones is then settled by comparing their coordinates."""
    ec = ked.cube_of(exp)
    starts = np.nonzero(np.r_[True, (np.diff(ec, axis=0) != 0).any(1)])[0]
    offset = {tuple(ec[s]): int(s) for s in starts}
    assert len(offset) == len(starts), "export_map() lists every cube in one run"
    slot = nb >> 20
    assert (slot == slot[:, :1]).all(), "a list lies in one cube"
    slot_cube = {}
    off = np.zeros(len(nb), np.int64)
    for i, (s, c) in enumerate(zip(slot[:, 0].tolist(), map(tuple, cube.tolist()))):
        assert slot_cube.setdefault(s, c) == c, "one cube per slot"
        off[i] = offset[c]
    return off[:, None] + (nb & (CAP_PER_SLOT - 1))


def _check_lists(exp, world_q, status, nbrs, want_judged, want_nbr, want_idx=None, what=""):
    """status classes, neighbour coordinates (and canonical indices) of every judged query; and -- independently of any reference --
    the product's own lists ascending in (d2 bits, canonical index)"""
    judged = np.isin(status, JUDGED)
    assert np.array_equal(judged, want_judged), (what, int(judged.sum()), int(want_judged.sum()))
    nb = _export_index(exp, nbrs[judged].astype(np.int64), ked.cube_of(want_nbr[judged][:, 0]))
    assert nb.min(initial=0) >= 0 and nb.max(initial=0) < len(exp), what
    got = exp[nb]
    bad = np.nonzero((got.view(np.uint32) != want_nbr[judged].view(np.uint32)).any(axis=(1, 2)))[0]
    assert len(bad) == 0, (what, f"{len(bad)} of {int(judged.sum())} lists differ; first: query {world_q[judged][bad[0]]}",
                           nb[bad[0]], got[bad[0]], want_nbr[judged][bad[0]])
    if want_idx is not None:
        assert np.array_equal(nb, want_idx[judged]), (what, "canonical indices")
    d2 = ked.d2_ref(world_q[judged][:, None, :], got)
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | nb.astype(np.uint64)
    assert (np.diff(key.astype(np.int64), axis=1) > 0).all(), (what, "lists ascending in (d2 bits, canonical index)")
    return int(judged.sum())


@pytest.mark.parametrize("name", NAMES)
def test_seam_b(oracle, gpu_slam_factory, name):
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, name)
    slam = _product(gpu_slam_factory, fam)
    q = fam.queries
    found, nbr, d2, idx = slam.nearest_k_search_surf(q, 5)
    slam.close()
    rf, ridx, rd2, rnbr = (a[:len(q)] for a in ref)
    of, onbr, od2, oidx, _ = om.knn(q, 5, use_grid=1)
    assert np.array_equal(found.astype(bool), rf) and np.array_equal(found, of)
    f = rf
    for want_d2, want_nbr, who in ((rd2, rnbr, "numpy"), (od2, onbr, "oracle")):
        assert np.array_equal(d2[f].view(np.uint32), want_d2[f].view(np.uint32)), (name, who, "d2 bits")
        assert np.array_equal(nbr[f].view(np.uint32), want_nbr[f].view(np.uint32)), (name, who, "neighbour coordinates")
    full = f & (rd2[:, 4] < 1e30)
    rows = _export_index(exp, idx[full].astype(np.int64), ked.cube_of(rnbr[full][:, 0]))
    assert np.array_equal(rows, ridx[full]), (name, "the indices Seam B returns are the canonical ones")
    key = (d2[full].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    assert (np.diff(key.astype(np.int64), axis=1) > 0).all(), (name, "lists ascending in (d2 bits, canonical index)")


def _register(slam, scan, pose):
    rc, pose_out, st = slam.register(scan, pose)
    assert rc == 0, slam.last_error()
    return st, slam.match_status(len(scan)), slam.neighbours(len(scan))


def _guess():
    from superodom_amd import synth
    return np.concatenate([[0.31, -0.17, 0.05], synth.quat_from_rotvec(np.array([0.004, -0.006, 0.013]))])


def _scan_under(pose, world):
    """scan points that the pose carries (up to rounding) onto the family's queries"""
    from superodom_amd import synth
    R = synth.quat_to_R(pose[3:])
    return np.ascontiguousarray(((world.astype(np.float64) - pose[:3]) @ R).astype(np.float32))


@pytest.mark.parametrize("pack", ["1", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_registration_sweep(oracle, soicp, gpu_slam_factory, monkeypatch, name, pack):
    """the chunked sweep (more than 4 096 queries), packed light chunks on / off; production and instrumented instantiation"""
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, name)
    monkeypatch.setenv("SOICP_KNN_PACK", pack)
    rf, ridx, rd2, rnbr = ref
    want_status = _expect_status(fam, ref)
    cfg1 = oracle.default_config(max_iterations=1)
    # -- identity pose: the world transform is exact, the numpy reference applies
    orc, _, _, corrs = om.register(scan, IDENTITY, cfg1, want_corrs=True)
    assert orc == 0
    assert np.array_equal(np.isin(corrs["status"], JUDGED), want_status == 0) and np.array_equal(corrs["status"] == 1, want_status == 1)
    slam = _product(gpu_slam_factory, fam)  # (a context per registration: the first registration of a context packs its light chunks)
    st, ms, nb = _register(slam, scan, IDENTITY)
    slam.close()
    assert not (st.flags & soicp.FLAG_QUERY_WAVES)
    _check_gate_sites(fam, ms, (name, pack))
    assert np.array_equal(ms, corrs["status"]), (name, "status bytes against the oracle")
    assert np.array_equal(ms == 1, want_status == 1) and np.array_equal(ms == 2, want_status == 2)
    n = _check_lists(exp, scan, ms, nb, want_status == 0, rnbr, ridx, (name, pack, "identity, numpy"))
    _check_lists(exp, scan, ms, nb, want_status == 0, corrs["nbr"].reshape(-1, 5, 3), None, (name, pack, "identity, oracle"))
    assert n > 100
    # -- a non-trivial guess: against the oracle's correspondences
    guess = _guess()
    scan_g = _scan_under(guess, scan)
    orc, _, _, cg = om.register(scan_g, guess, cfg1, want_corrs=True)
    assert orc == 0
    slam = _product(gpu_slam_factory, fam)
    st, ms_g, nb_g = _register(slam, scan_g, guess)
    slam.close()
    assert np.array_equal(ms_g, cg["status"]), (name, "status bytes against the oracle, guess")
    jg = np.isin(ms_g, JUDGED)
    want_g = cg["nbr"].reshape(-1, 5, 3)
    got = exp[_export_index(exp, nb_g[jg].astype(np.int64), ked.cube_of(want_g[jg][:, 0]))]
    assert np.array_equal(got.view(np.uint32), want_g[jg].view(np.uint32)), (name, pack, "guess: neighbour coordinates")
    # the product's sweep leaves no d2: the oracle's d2 belong to these very lists (same points, same order), and under them the
    # product's canonical indices must break every tie
    rows_g = _export_index(exp, nb_g[jg].astype(np.int64), ked.cube_of(want_g[jg][:, 0]))
    key = (cg["d2"][jg].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows_g.astype(np.uint64)
    assert (np.diff(key.astype(np.int64), axis=1) > 0).all(), (name, pack, "guess: (oracle d2 bits, canonical index) ascending")
    # -- the instrumented instantiation: same lists, and the branch the family aims at was taken
    monkeypatch.setenv("SOICP_ABLATE", ABLATE_STATS_ONLY)
    prof = _product(gpu_slam_factory, fam, time_kernels=2)
    monkeypatch.delenv("SOICP_ABLATE")
    st, ms_p, nb_p = _register(prof, scan, IDENTITY)
    t = prof.timing()
    prof.close()
    assert np.array_equal(ms_p, ms) and np.array_equal(nb_p[np.isin(ms, JUDGED)], nb[np.isin(ms, JUDGED)]), (name, "instrumented sweep")
    counters = dict(group_passes=t.knn_group_passes, fallback_lanes=t.knn_fallback_lanes, packed_rows=t.knn_packed_rows,
                    rows_too_many_runs=t.knn_packed_rows_too_many_runs, rows_tile_full=t.knn_packed_rows_tile_full, packed_kept=t.knn_packed_kept)
    counters["pack_holds"] = t.knn_pack_holds
    print(f"{name} pack={pack}: {counters}")
    assert t.knn_group_passes > 0
    aim = fam.info["aim"]
    if pack == "1":
        assert t.knn_packed_rows > 0, "light chunks were packed"
    if aim in ("fallback", "dense") and (pack == "0" or name != "near_ties"):
        # eight equal / near-equal distances no key can order, blocks beyond the key's index field: lanes of ordinary chunks that
        # no pass certifies and the exact scan answers
        assert t.knn_fallback_lanes > 0, counters
    if name == "near_ties" and pack == "0":
        assert t.knn_fallback_lanes == len(fam.queries), "NO site can be certified: every one of its queries goes to the exact scan"
    if name == "near_ties" and pack == "1":
        # every site is a light chunk of its own; what a packed row leaves to the exact scan is counted on the device and read by
        # the host's packing policy alone: all 363 queries of 4 200 left over is more than its 3 % and must trip it
        assert t.knn_fallback_lanes == 0 and t.knn_pack_holds == 1, counters
    if aim == "dense" and pack == "1":
        assert t.knn_packed_rows_tile_full > 0, counters  # rows that keep more than their quarter of the tile


@pytest.mark.parametrize("name", NAMES)
def test_query_wave_sweep(oracle, soicp, gpu_slam_factory, name):
    """the same queries in scans of at most 4 096: one wavefront per query"""
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, name)
    slam = _product(gpu_slam_factory, fam)
    q = fam.queries
    for lo in range(0, len(q), 4096):
        part = np.ascontiguousarray(q[lo:lo + 4096])
        rf, ridx, rd2, rnbr = (a[lo:lo + len(part)] for a in ref)
        want_status = _expect_status(fam, (rf, ridx, rd2, rnbr))
        st, ms, nb = _register(slam, part, IDENTITY)
        assert st.flags & soicp.FLAG_QUERY_WAVES, hex(st.flags)
        _check_gate_sites(fam, ms, (name, "query waves"))
        assert np.array_equal(ms == 1, want_status == 1) and np.array_equal(ms == 2, want_status == 2)
        _check_lists(exp, part, ms, nb, want_status == 0, rnbr, ridx, (name, lo, "query waves, numpy"))
        orc, _, _, corrs = om.register(part, IDENTITY, oracle.default_config(max_iterations=1), want_corrs=True)
        assert orc == 0 and np.array_equal(ms, corrs["status"])
        _check_lists(exp, part, ms, nb, want_status == 0, corrs["nbr"].reshape(-1, 5, 3), None, (name, lo, "query waves, oracle"))
    slam.close()


@pytest.mark.parametrize("name", NAMES)
def test_batched_sweep(oracle, soicp, gpu_slam_factory, name):
    """three hypotheses from the same guess (the batched sweep starts with the full pass): each equals the single registration --
    rejection and observability histograms (the status bytes, counted), costs and the pose, bit for bit -- and the oracle's histograms"""
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, name)
    guess = _guess()
    scan_g = _scan_under(guess, scan)
    slam = _product(gpu_slam_factory, fam)
    rc, pose, st = slam.register(scan_g, guess)
    assert rc == 0
    ok, rcs, poses, sts = slam.register_batch(scan_g, np.stack([guess, guess, guess]))
    slam.close()
    assert ok == 3 and (rcs == 0).all()
    orc, _, ost, _ = om.register(scan_g, guess, oracle.default_config(max_iterations=1))
    for h in range(3):
        assert sts[h].n_iterations == 1
        assert_same_bits(sts[h], st, (name, h), omit=("uncertainty",))  # (from the call before: the batch follows the single registration)
        assert np.array_equal(poses[h], pose)
        assert_follows_oracle(sts[h], ost, (name, h))


def _prof_sweep(make, monkeypatch, fam, scan, pack):
    monkeypatch.setenv("SOICP_KNN_PACK", pack)
    monkeypatch.setenv("SOICP_ABLATE", ABLATE_STATS_ONLY)
    prof = _product(make, fam, time_kernels=2)
    monkeypatch.delenv("SOICP_ABLATE")
    st, ms, nb = _register(prof, scan, IDENTITY)
    t = prof.timing()
    prof.close()
    return ms, nb, t


@pytest.mark.parametrize("pack", ["1", "0"])
def test_the_2048_candidate_limit_sends_a_block_to_the_exact_scan_and_one_candidate_less_does_not(oracle, gpu_slam_factory, monkeypatch, pack):
    """The same sites with 2047 / 2048 candidates in the block and with 2049: the first are selected by keys (the index field holds
    2048 positions) -- no lane reaches the exact scan --, of the second EVERY lane of an ordinary chunk does.  (Queries of a dense 0.1 m
    lattice are certified by the near pass: the 5th neighbour lies at ~0.1 m, the block's faces at 0.39 m or more.)"""
    for sites, over in ((((2047, 40), (2048, 40), (2047, 12), (2048, 12)), False), (((2049, 40), (2049, 12), (2049, 33)), True)):
        fam = ked.dense(seed=11, n_cubes=2, site_list=sites, name="dense_edge")
        slam = _product(gpu_slam_factory, fam)
        exp = slam.export_map()
        slam.close()
        q = fam.queries
        rf, ridx, rd2, rnbr = ked.brute_knn(exp, q)
        ms, nb, t = _prof_sweep(gpu_slam_factory, monkeypatch, fam, q, pack)
        assert rf.all() and np.isin(ms, JUDGED).all()
        _check_lists(exp, q, ms, nb, np.ones(len(q), bool), rnbr, ridx, ("dense_edge", sites, pack))
        ordinary = sum(nq for cu, h, k, nq in fam.info["sites"] if pack == "0" or nq > 16)  # (a packed row's leftovers are not counted here)
        print(f"dense_edge {sites} pack={pack}: fallback lanes {t.knn_fallback_lanes}, queries in ordinary chunks {ordinary}")
        assert t.knn_fallback_lanes == (ordinary if over else 0), (sites, pack, t.knn_fallback_lanes, ordinary)


@pytest.mark.parametrize("mode", ["instrumented", "production"])
def test_chunks_binned_ahead_under_another_pose(oracle, soicp, gpu_slam_factory, monkeypatch, mode):
    """Chunks that are not compact (knn_edge_data.xruns): scan B is announced, registration A -- 100 m away, where B meets no cube --
    bins it ahead under its own pose, B is then swept under the identity: chunks of 64 queries from all over a lattice (more than 32
    x-runs: the group shrinks to the leader's cells), a light chunk of 9 (more than 16 x-runs: the packed row is handed back) and
    lanes of one chunk in eight cubes.  Whether a scan IS binned ahead is decided by the host's timing (300 us from the announcement
    to the registration's launches): the pair is repeated until it was, every repetition is checked."""
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, "xruns")
    if mode == "instrumented":
        monkeypatch.setenv("SOICP_ABLATE", ABLATE_STATS_ONLY)
    slam = _product(gpu_slam_factory, fam, **({"time_kernels": 2} if mode == "instrumented" else {}))
    monkeypatch.delenv("SOICP_ABLATE", raising=False)
    n1 = fam.info["n_one"]
    A = slam.host_alloc_like(fam.info["scan_a"])
    parts = [(slam.host_alloc_like(fam.queries[:n1]), tuple(a[:n1] for a in ref)), (slam.host_alloc_like(fam.queries[n1:]), tuple(a[n1:2 * n1] for a in ref))]
    cfg1 = oracle.default_config(max_iterations=1)
    want = []
    for B, r in parts:
        orc, _, _, corrs = om.register(B, IDENTITY, cfg1, want_corrs=True)
        assert orc == 0
        want.append((_expect_status(fam, r), corrs))
    ahead = [0, 0]
    for attempt in range(16):
        for k, (B, r) in enumerate(parts):
            slam.stage_scan(B)
            rc, _, _ = slam.register(A, fam.info["pose_a"])
            assert rc == 0, slam.last_error()
            st, ms, nb = _register(slam, B, IDENTITY)
            assert st.flags & soicp.FLAG_STAGED_SCAN
            ahead[k] += bool(st.flags & soicp.FLAG_BINNED_AHEAD)
            ws, corrs = want[k]
            assert np.array_equal(ms, corrs["status"]), (mode, attempt, k)
            assert np.array_equal(ms == 1, ws == 1) and np.array_equal(ms == 2, ws == 2)
            n = _check_lists(exp, B, ms, nb, ws == 0, r[3], r[1], (mode, attempt, k, "numpy"))
            _check_lists(exp, B, ms, nb, ws == 0, corrs["nbr"].reshape(-1, 5, 3), None, (mode, attempt, k, "oracle"))
            assert n > 1000
        if min(ahead) >= 2:
            break
    print(f"{mode}: binned ahead {ahead} times in {attempt + 1} rounds")
    assert min(ahead) >= 1, ("the scans were never binned ahead: the path was not exercised", ahead)
    if mode == "instrumented":
        t = slam.timing()
        print(dict(fallback_lanes=t.knn_fallback_lanes, packed_rows=t.knn_packed_rows, rows_too_many_runs=t.knn_packed_rows_too_many_runs,
                   rows_tile_full=t.knn_packed_rows_tile_full, group_passes=t.knn_group_passes))
        assert t.knn_packed_rows_too_many_runs > 0, "a packed row with more than 16 x-runs was handed back"
        assert t.knn_fallback_lanes > 0
    slam.close()


def test_a_block_face_on_the_cube_boundary_does_not_limit_the_certificate(oracle, gpu_slam_factory, monkeypatch):
    """knn_edge_data.boundary_block: one chunk whose near block begins at the cube's own face.  That face has nothing of the cube behind it
    and must not enter the cover distance: the near pass certifies all 40 queries -- ONE group pass, no exact scan.  (Counting the face
    in makes the cover distance the few centimetres to it, and every query takes a second, full pass: same lists, twice the work.)"""
    fam = ked.boundary_block()
    slam = _product(gpu_slam_factory, fam)
    exp = slam.export_map()
    slam.close()
    q = fam.queries
    rf, ridx, rd2, rnbr, tail = ked.brute_knn(exp, q, n_tail=3)
    assert rf.all() and (rd2[:, 4] < 0.12).all() and (tail[:, 5] - tail[:, 4] > 1e-4).all(), "5th neighbour well inside half a cell, 6th clearly behind it"
    nc, cell = ked.grid_cells(fam.plane_res)
    half = np.floor((q.astype(np.float64) + 25.0) % 50.0 / (cell / 2)).astype(np.int64)
    assert (half == half[0]).all() and half[0][0] == 0, "one half-cell octant, in the first cell of the cube"
    ms, nb, t = _prof_sweep(gpu_slam_factory, monkeypatch, fam, q, "0")
    _check_lists(exp, q, ms, nb, np.ones(len(q), bool), rnbr, ridx, "boundary_block")
    print(f"boundary_block: group passes {t.knn_group_passes}, fallback lanes {t.knn_fallback_lanes}")
    assert t.knn_group_passes == 1 and t.knn_fallback_lanes == 0


# ------------------------------------------------------------------------------------------------------------------------
# the gate family binned ahead; Seam B at every k; scan rows that are not finite
# ------------------------------------------------------------------------------------------------------------------------
def test_gate_sites_binned_ahead_at_0_8(oracle, soicp, gpu_slam_factory):
    """The pattern of test_chunks_binned_ahead_under_another_pose with the gate sites of the coarsest grid (planeRes 0.8: cells of
    1.5625 m, gate radius 1.549 m) as scan B: binned under pose A, where it meets no cube, B is cut into chunks of 64 in arrival order
    -- queries of sites metres and cubes apart in one chunk, the largest block-local coordinates the selection key sees.  Same
    repetition rule, same requirement that the scan WAS binned ahead at least once."""
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, "gate_edge_0.8")
    slam = _product(gpu_slam_factory, fam)
    A, B = slam.host_alloc_like(fam.info["scan_a"]), slam.host_alloc_like(scan)
    orc, _, _, corrs = om.register(B, IDENTITY, oracle.default_config(max_iterations=1), want_corrs=True)
    assert orc == 0
    ws = _expect_status(fam, ref)
    ahead = 0
    for attempt in range(16):
        slam.stage_scan(B)
        rc, _, _ = slam.register(A, fam.info["pose_a"])
        assert rc == 0, slam.last_error()
        st, ms, nb = _register(slam, B, IDENTITY)
        assert st.flags & soicp.FLAG_STAGED_SCAN
        ahead += bool(st.flags & soicp.FLAG_BINNED_AHEAD)
        _check_gate_sites(fam, ms, ("binned ahead", attempt))
        assert np.array_equal(ms, corrs["status"]), attempt
        assert np.array_equal(ms == 1, ws == 1) and np.array_equal(ms == 2, ws == 2)
        n = _check_lists(exp, B, ms, nb, ws == 0, ref[3], ref[1], (attempt, "numpy"))
        _check_lists(exp, B, ms, nb, ws == 0, corrs["nbr"].reshape(-1, 5, 3), None, (attempt, "oracle"))
        assert n == 104
        if ahead >= 2:
            break
    slam.close()
    print(f"gate_edge_0.8: binned ahead {ahead} times in {attempt + 1} rounds")
    assert ahead >= 1, "the scan was never binned ahead: the path was not exercised"


@pytest.mark.parametrize("name", NAMES)
def test_seam_b_every_k(oracle, gpu_slam_factory, name):
    """k = 1 .. 4: found flags, d2 bits, neighbour coordinates and canonical indices against the oracle on EVERY query and against the
    numpy reference (the first k of its 5-list where the cube holds five points -- which the product's own 5-list must equal too --,
    brute_knn(k=k) itself where it holds fewer).  A cube of fewer than k points leaves the reference's buffer: unfilled slots name the
    cube's first point with d2 0, slot k - 1 carries FLT_MAX.  A query without a cube: all zero, index -1."""
    fam, exp, om, scan, ref = _setup(oracle, gpu_slam_factory, name)
    q = fam.queries
    rf5, ridx5, rd25, rnbr5 = (a[:len(q)] for a in ref)
    counts = ked.cell_counts(exp, q)
    assert np.array_equal(counts > 0, rf5)
    few = (counts > 0) & (counts < 5)
    ec = ked.cube_of(exp)
    first = {tuple(ec[s]): exp[s] for s in np.nonzero(np.r_[True, (np.diff(ec, axis=0) != 0).any(1)])[0]}  # (export_map() lists a cube in one run)
    slam = _product(gpu_slam_factory, fam)
    f5, nbr5, d25, idx5 = slam.nearest_k_search_surf(q, 5)
    for k in (1, 2, 3, 4):
        found, nbr, d2, idx = slam.nearest_k_search_surf(q, k)
        assert nbr.shape == (len(q), k, 3)
        # -- the oracle, every query
        of, onbr, od2, oidx, _ = om.knn(q, k, use_grid=1)
        assert np.array_equal(found, of) and np.array_equal(found.astype(bool), rf5), (name, k)
        f = rf5
        assert np.array_equal(d2[f].view(np.uint32), od2[f].view(np.uint32)), (name, k, "oracle", "d2 bits")
        assert np.array_equal(nbr[f].view(np.uint32), onbr[f].view(np.uint32)), (name, k, "oracle", "neighbour coordinates")
        # -- numpy
        wd2, wnbr, widx = rd25[:, :k].copy(), rnbr5[:, :k].copy(), ridx5[:, :k].copy()
        if few.any():
            _, widx[few], wd2[few], wnbr[few] = ked.brute_knn(exp, q[few], k=k)
        assert np.array_equal(d2[f].view(np.uint32), wd2[f].view(np.uint32)), (name, k, "numpy", "d2 bits")
        assert np.array_equal(nbr[f].view(np.uint32), wnbr[f].view(np.uint32)), (name, k, "numpy", "neighbour coordinates")
        rows = _export_index(exp, idx[f].astype(np.int64), ked.cube_of(wnbr[f][:, 0]))
        assert np.array_equal(rows, widx[f]), (name, k, "canonical indices")
        # -- the first k of the product's own 5-list
        full = counts >= 5
        assert np.array_equal(d2[full].view(np.uint32), d25[full][:, :k].view(np.uint32)) and np.array_equal(idx[full], idx5[full][:, :k]) and \
            np.array_equal(nbr[full].view(np.uint32), nbr5[full][:, :k].view(np.uint32)), (name, k, "the k-list is the head of the 5-list")
        # -- a cube of fewer than k points
        for i in np.nonzero((counts > 0) & (counts < k))[0]:
            m = counts[i]
            p0 = first[tuple(ked.cube_of(q[i]))]
            assert (nbr[i, m:] == p0).all() and (d2[i, m:k - 1] == 0).all() and d2[i, k - 1] == ked.FLT_MAX, (name, k, i, nbr[i], d2[i])
            assert (idx[i, m:] & (CAP_PER_SLOT - 1) == 0).all() and (idx[i, m:] >> 20 == idx[i, 0] >> 20).all(), (name, k, i, idx[i])
        for i in np.nonzero(counts == k)[0]:
            assert d2[i, k - 1] < 1e30, "a cube of exactly k points fills every slot"
        # -- no cube
        assert (nbr[~f] == 0).all() and (d2[~f] == 0).all() and (idx[~f] == -1).all() and (found[~f] == 0).all(), (name, k)
    slam.close()
    if name.startswith("faces"):
        assert {1, 2, 3, 4} <= set(counts.tolist()), "the cubes of 1 .. 4 points"


_nonfinite = {}


def _nonfinite_case(oracle, make, n_rows=None):
    """the faces scan (padded by _scan_of; its first n_rows rows) with the non-finite rows in it, and the oracle's registration of
    that very scan"""
    if n_rows not in _nonfinite:
        fam, exp, om, scan, ref = _setup(oracle, make, "faces")
        bad, rows = ked.nonfinite_rows(scan[:n_rows])
        orc, _, ost, corrs = om.register(bad, IDENTITY, oracle.default_config(max_iterations=1), want_corrs=True)
        assert orc == 0 and (corrs["status"][rows] == 1).all()
        assert ref[0][:len(bad)][rows].sum() > 60, "most of the rows had a cube before"
        _nonfinite[n_rows] = (fam, exp, bad, rows, ost, corrs)
    return _nonfinite[n_rows]


def _check_nonfinite(exp, bad, rows, st, ms, nb, ost, corrs, what):
    """the named rows are outside every window; every other row has the oracle's status and the oracle's list"""
    assert (ms[rows] == 1).all(), (what, ms[rows])
    assert np.array_equal(ms, corrs["status"]), (what, np.nonzero(ms != corrs["status"])[0][:10])
    judged = np.isin(corrs["status"], JUDGED)
    assert not judged[rows].any()
    n = _check_lists(exp, bad, ms, nb, judged, corrs["nbr"].reshape(-1, 5, 3), None, what)
    assert n > 1000
    assert_follows_oracle(st, ost, what)


@pytest.mark.parametrize("pack", ["1", "0"])
def test_nonfinite_rows_in_the_chunked_sweep(oracle, soicp, gpu_slam_factory, monkeypatch, pack):
    fam, exp, bad, rows, ost, corrs = _nonfinite_case(oracle, gpu_slam_factory)
    monkeypatch.setenv("SOICP_KNN_PACK", pack)
    slam = _product(gpu_slam_factory, fam)
    st, ms, nb = _register(slam, bad, IDENTITY)
    slam.close()
    assert not (st.flags & soicp.FLAG_QUERY_WAVES)
    _check_nonfinite(exp, bad, rows, st, ms, nb, ost, corrs, ("chunked", pack))


def test_nonfinite_rows_in_the_query_waves(oracle, soicp, gpu_slam_factory):
    fam, exp, bad, rows, ost, corrs = _nonfinite_case(oracle, gpu_slam_factory, 4096)
    assert len(bad) == 4096 and rows[-1] == 4095
    slam = _product(gpu_slam_factory, fam)
    st, ms, nb = _register(slam, bad, IDENTITY)
    slam.close()
    assert st.flags & soicp.FLAG_QUERY_WAVES
    _check_nonfinite(exp, bad, rows, st, ms, nb, ost, corrs, "query waves")


def test_nonfinite_rows_in_a_scan_binned_ahead(oracle, soicp, gpu_slam_factory):
    """announced, binned beside a registration of the clean scan, then registered (repeated until it WAS binned ahead, as above)"""
    fam, exp, bad, rows, ost, corrs = _nonfinite_case(oracle, gpu_slam_factory)
    slam = _product(gpu_slam_factory, fam)
    A, B = slam.host_alloc_like(_setup(oracle, gpu_slam_factory, "faces")[3]), slam.host_alloc_like(bad)
    ahead = 0
    for attempt in range(16):
        slam.stage_scan(B)
        rc, _, _ = slam.register(A, IDENTITY)
        assert rc == 0, slam.last_error()
        st, ms, nb = _register(slam, B, IDENTITY)
        assert st.flags & soicp.FLAG_STAGED_SCAN
        ahead += bool(st.flags & soicp.FLAG_BINNED_AHEAD)
        _check_nonfinite(exp, B, rows, st, ms, nb, ost, corrs, ("binned ahead", attempt))
        if ahead >= 2:
            break
    slam.close()
    print(f"non-finite rows: binned ahead {ahead} times in {attempt + 1} rounds")
    assert ahead >= 1, "the scan was never binned ahead: the path was not exercised"


def test_nonfinite_rows_in_a_resident_scan_and_a_batch(oracle, soicp, gpu_slam_factory):
    """so_icp_register_dev and a batch of three equal the registration of the host scan, bit for bit"""
    fam, exp, bad, rows, ost, corrs = _nonfinite_case(oracle, gpu_slam_factory)
    slam = _product(gpu_slam_factory, fam)
    rc, pose, st = slam.register(bad, IDENTITY)
    assert rc == 0, slam.last_error()
    d_scan, n = slam.upload_scan(bad)
    rc, pose_d, st_d = slam.register_dev(d_scan, n, IDENTITY)
    assert rc == 0, slam.last_error()
    ms, nb = slam.match_status(n), slam.neighbours(n)
    _check_nonfinite(exp, bad, rows, st_d, ms, nb, ost, corrs, "resident")
    assert_same_bits(st_d, st, "resident", omit=CARRIED_OVER_FIELDS)
    assert np.array_equal(pose_d, pose)
    rc, pose2, st2 = slam.register(bad, IDENTITY)  # (the call before the batch: what its carried-over fields follow)
    assert rc == 0
    ok, rcs, poses, sts = slam.register_batch(bad, np.stack([IDENTITY, IDENTITY, IDENTITY]))
    slam.free_scan(d_scan)
    slam.close()
    assert ok == 3 and (rcs == 0).all()
    for h in range(3):
        assert_same_bits(sts[h], st2, ("batch", h), omit=("uncertainty",))
        assert np.array_equal(poses[h], pose2)
        assert_follows_oracle(sts[h], ost, ("batch", h))
