"""-m gpu: the first stage of a registration at its edges, on every front end.  The sampling rule (LidarSlam.cpp:346-359) is written at
three sites of the device code -- scan_keys_kernel (plain, batched, and with the query split's re-indexing), the prologue of a scan
binned ahead (knn_plane_kernel's begin, reg_begin_prebinned_kernel under the instrumented build) and the lanes of knn_query_wave_kernel
-- and derived at a fourth, the share partition of the query waves.  The pairs (n, max_surface_features) of sampling_edge_data.PAIRS
(their census is asserted on the CPU by test_sampling_edges_host.py) go through all of them: status bytes against orc_should_process
for EVERY index, and status bytes, neighbour lists, histograms, iteration counts and pose bits identical across the front ends and
following the oracle.  Then the bucket sizes of the binning (binning_edge_data.py) and the whole-cell key of a map with more than
2046 occupied cubes.  Product against product is bit equality; product against oracle goes through helpers.py."""
import contextlib
import os

import numpy as np
import pytest

import binning_edge_data as bed
import knn_edge_data as ked
import sampling_edge_data as sed
from helpers import (CARRIED_OVER_FIELDS, assert_follows_oracle, assert_rank_follows_single, assert_same_bits, bits_field, chain_deltas,
                     in_threads, stats_of)
from superodom_amd import synth
from test_gpu_knn_edges import ABLATE_STATS_ONLY, IDENTITY, JUDGED, _check_lists
from test_gpu_sequence import _check_run

pytestmark = pytest.mark.gpu

DROPPED = sed.DROPPED
FEW_KEPT_OMIT = ("lm_iterations", "num_successful_steps", "termination", "final_cost")  # fewer than 100 kept points: status bytes, histograms, counts
CARRIER_N = 4200  # the registration a staged scan is binned ahead behind: a chunked sweep of its own


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class FrontEnd:
    """One way a scan reaches the sweep: a context (its switches are read by so_icp_create) and an entry."""

    def __init__(self, name, make, sc, env=None, entry="register", **cfg):
        self.name, self.entry, self.chunked_timed = name, entry, cfg.get("time_kernels", 0) >= 2
        with _env(**(env or {})):
            self.slam = make(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=1, **cfg)
        self.slam.add_surf_point_cloud(sc.map_points)
        self.pinned = {}
        if entry == "staged":
            self.carrier = self.slam.host_alloc_like(np.ascontiguousarray(sc.scan(1)[:CARRIER_N]))
            self.carrier_pose = sc.guess(1)

    def run(self, soicp, scan, guess, msf, max_iterations, key=None):
        """-> (Stats, pose, status bytes, neighbour lists, growth of (knn_queries, knn_launches))"""
        s = self.slam
        s.set_max_surface_features(msf); s.set_max_iterations(max_iterations)
        n = len(scan)
        if self.entry == "register":
            t0 = s.timing()
            rc, pose, st = s.register(scan, guess)
        elif self.entry == "resident":
            d, _ = s.upload_scan(scan)
            t0 = s.timing()
            rc, pose, st = s.register_dev(d, n, guess)
            s.free_scan(d)
        else:
            # announced, then binned ahead behind the registration in flight (the carrier's), under the carrier's guess.  Whether that
            # happens is decided by the host's timing (300 us from the announcement to the carrier's launches): repeated until it did.
            key = key if key is not None else (n, scan[:8].tobytes())
            if key not in self.pinned:
                self.pinned[key] = s.host_alloc_like(scan)
            B = self.pinned[key]
            for attempt in range(16):
                s.stage_scan(B)
                s.register(self.carrier, self.carrier_pose)
                t0 = s.timing()
                rc, pose, st = s.register(B, guess)
                assert st.flags & soicp.FLAG_STAGED_SCAN, (self.name, hex(st.flags))
                if st.flags & soicp.FLAG_BINNED_AHEAD:
                    break
            assert st.flags & soicp.FLAG_BINNED_AHEAD, (self.name, "the scan was never binned ahead: the path was not exercised", hex(st.flags))
        assert rc == 0, (self.name, rc, s.last_error())
        t1 = s.timing()
        return st, pose, s.match_status(n), s.neighbours(n), (t1.knn_queries - t0.knn_queries, t1.knn_launches - t0.knn_launches)


@pytest.fixture(scope="module")
def world(oracle, soicp, gpu_slam_factory):
    sc = synth.Scene("small")
    fes = [FrontEnd("default", gpu_slam_factory, sc),
           FrontEnd("chunked", gpu_slam_factory, sc, env={"SOICP_QUERY_WAVES": "0"}, time_kernels=2),
           FrontEnd("staged", gpu_slam_factory, sc, env={"SOICP_QUERY_WAVES": "0"}, entry="staged"),
           # the instrumented build keeps the prologue out of the sweep: reg_begin_prebinned_kernel writes the DROPPED bytes
           FrontEnd("staged, instrumented", gpu_slam_factory, sc, env={"SOICP_ABLATE": ABLATE_STATS_ONLY}, entry="staged", time_kernels=2),
           FrontEnd("resident", gpu_slam_factory, sc, entry="resident")]
    exp = fes[0].slam.export_map()
    om = oracle.OracleMap(plane_res=sc.plane_res)
    assert om.add_surf(exp, raw=True) == len(exp)
    yield sc, fes, exp, om
    for fe in fes:
        fe.slam.close()


_scans = {}


def _scan(sc, n, index=0):
    if (n, index) not in _scans:
        _scans[(n, index)] = sed.scan_of(sc, n, seed=1000 + n % 997 + index, index=index)
    return _scans[(n, index)]


def _oracle_status(corrs):
    return np.where(corrs["status"] < 0, DROPPED, corrs["status"]).astype(np.uint8)


def _same_registration(a, b, tag):
    """two front ends: status bytes, neighbour lists of the judged queries, every deterministic statistic and the pose, to the bit"""
    st_a, pose_a, ms_a, nb_a, _ = a
    st_b, pose_b, ms_b, nb_b, _ = b
    assert np.array_equal(ms_a, ms_b), (tag, "status bytes", np.nonzero(ms_a != ms_b)[0][:8])
    j = np.isin(ms_a, JUDGED)
    assert np.array_equal(nb_a[j], nb_b[j]), (tag, "neighbour lists")
    assert_same_bits(st_a, st_b, tag, omit=CARRIED_OVER_FIELDS)  # (the contexts have different call histories)
    assert pose_a.tobytes() == pose_b.tobytes(), (tag, "pose bits")


@pytest.mark.parametrize("pair", list(sed.PAIRS), ids=sed.pair_id)
def test_pair_on_every_front_end(oracle, soicp, world, pair):
    sc, fes, exp, om = world
    n, msf = pair
    want = sed.PAIRS[pair]
    scan, guess = _scan(sc, n), sc.guess(0)
    keep = sed.keeps(n, msf)
    kept = int(keep.sum())
    assert kept == want["kept"]
    orc, _, ost1, corrs = om.register(scan, guess, oracle.default_config(max_iterations=1, max_surface_features=msf), want_corrs=True)
    assert orc == 0
    want_status = _oracle_status(corrs)
    assert np.array_equal(want_status == DROPPED, ~keep), "orc_should_process, every index"
    front_ends = fes  # (all of them single contexts: the two 100 000-point pairs included)
    first = None
    for fe in front_ends:
        res = fe.run(soicp, scan, guess, msf, 1)
        st, pose, ms, nb, (grew_q, grew_l) = res
        tag = (pair, fe.name)
        assert np.array_equal(ms == DROPPED, ~keep), (tag, "254 exactly where the rule drops", np.nonzero((ms == DROPPED) != ~keep)[0][:8])
        assert np.array_equal(ms, want_status), (tag, "status bytes against the oracle", np.nonzero(ms != want_status)[0][:8])
        assert bool(st.flags & soicp.FLAG_QUERY_WAVES) == (sed.takes_query_waves(n, msf) and fe.name in ("default", "resident")), (tag, hex(st.flags))
        assert st.n_iterations == 1 and sum(st.iterations[0].reject_hist) == kept, (tag, list(st.iterations[0].reject_hist))
        if fe.chunked_timed:
            assert (grew_q, grew_l) == (kept, 1), (tag, "knn_queries grows by the kept count per sweep", grew_q, grew_l)
        assert_follows_oracle(st, ost1, tag, omit=FEW_KEPT_OMIT if kept < 100 else ())
        if first is None:
            first = res
        else:
            _same_registration(res, first, (pair, fe.name, "against", front_ends[0].name))
    if kept < 100:
        return
    orc, opose, ost, _ = om.register(scan, guess, oracle.default_config(max_iterations=5, max_surface_features=msf))
    assert orc == 0
    first = None
    for fe in front_ends:
        res = fe.run(soicp, scan, guess, msf, 5)
        st, pose, ms, nb, (grew_q, grew_l) = res
        tag = (pair, fe.name, "5 outer iterations")
        assert_follows_oracle(st, ost, tag, pose=pose, opose=opose)
        assert np.array_equal(ms == DROPPED, ~keep), tag
        if fe.chunked_timed:
            assert (grew_q, grew_l) == (kept * st.n_iterations, st.n_iterations), (tag, grew_q, grew_l, st.n_iterations)
        if first is None:
            first = res
        else:
            _same_registration(res, first, tag)


def _to_world(scan, pose):
    R = synth.quat_to_R(pose[3:])
    return np.ascontiguousarray((scan.astype(np.float64) @ R.T + pose[:3]).astype(np.float32))


@pytest.mark.parametrize("pair", sed.LATE_PAIRS, ids=sed.pair_id)
def test_kept_points_of_the_later_trips_by_name(oracle, soicp, world, pair):
    """The kept points beyond offset 63 of their share are searched in the second / third trip of knn_query_wave_kernel's share loop,
    with coordinates that trip loads itself (`base != i_lo`).  A trip that kept the first trip's registers would search lane l's point of
    the FIRST trip -- 64 (128) scan points earlier, whose list is another one (asserted) -- and leave that list here.  The scan is given
    in the world frame and registered under the identity, where the transform is exact and the numpy reference applies."""
    sc, fes, exp, om = world
    n, msf = pair
    c = sed.census(n, msf)
    late = c["late"]
    assert len(late) == sed.PAIRS[pair]["late"] == 25 and set(c["late_offsets"].tolist()) == {sed.PAIRS[pair]["late_at"]}
    scan = _to_world(_scan(sc, n), sc.gt_pose(0))
    rf, ridx, rd2, rnbr = ked.brute_knn(exp, scan[late])
    gate = np.float64(np.float32(3) * np.float32(sc.plane_res))
    judged = rf & (rd2[:, 4].astype(np.float64) <= gate)
    assert judged.sum() >= 20, "the late points have their five neighbours inside the gate"
    trip = sed.PAIRS[pair]["late_at"] // 64
    twin = late - 64 * trip  # the point the same lane held in the first trip
    tf, tidx, _, _ = ked.brute_knn(exp, scan[twin])
    assert (ridx[judged] != tidx[judged]).any(axis=1).all(), "the first trip's point of the lane has another neighbour list"
    qw = fes[0].run(soicp, scan, IDENTITY, msf, 1)
    ch = fes[1].run(soicp, scan, IDENTITY, msf, 1)
    assert qw[0].flags & soicp.FLAG_QUERY_WAVES and not (ch[0].flags & soicp.FLAG_QUERY_WAVES)
    for (st, pose, ms, nb, _), who in ((qw, "query waves"), (ch, "chunked sweep")):
        assert np.array_equal(ms == DROPPED, ~sed.keeps(n, msf)), (pair, who)
        assert np.array_equal(ms[late] == 2, rf & ~judged) and np.array_equal(ms[late] == 1, ~rf), (pair, who)
        _check_lists(exp, scan[late], ms[late], nb[late], judged, rnbr, ridx, (pair, who, "late kept points, numpy"))
    j = np.isin(qw[2], JUDGED)
    assert np.array_equal(qw[2], ch[2]) and np.array_equal(qw[3][j], ch[3][j]), (pair, "query waves against the chunked sweep, every query")
    assert np.array_equal(qw[3][late][judged], ch[3][late][judged])


def test_status_bytes_of_the_registration_before_do_not_survive(oracle, soicp, world):
    """the status buffer is reused: a point dropped by one registration and kept by the next must lose its 254, on every front end that
    writes the DROPPED bytes in a place of its own"""
    sc, fes, exp, om = world
    long = _scan(sc, 13734)
    guess = sc.guess(0)
    steps = ((4097, 0), (4097, -1), (13734, 210), (6401, 100))
    for fe in fes:
        for n, msf in steps:
            st, pose, ms, nb, _ = fe.run(soicp, np.ascontiguousarray(long[:n]), guess, msf, 1, key=("stale", n))
            keep = sed.keeps(n, msf)
            assert np.array_equal(ms == DROPPED, ~keep), (fe.name, n, msf, int((ms == DROPPED).sum()), int((~keep).sum()))
            if (n, msf) == (4097, 0):
                assert (ms == DROPPED).all()
            if (n, msf) == (4097, -1):
                assert not (ms == DROPPED).any()
            assert sum(st.iterations[0].reject_hist) == int(keep.sum())


@pytest.mark.parametrize("pair", [(13734, 210), (5000, 4095)], ids=sed.pair_id)
def test_register_sequence_frames_equal_single_registrations(oracle, soicp, gpu_slam_factory, pair):
    """the chained BEGIN launch on both sweeps: every frame is so_icp_register from the guess the run reports, to the bit"""
    n, msf = pair
    sc = synth.Scene("small")
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=msf, max_iterations=5)
    slam, plain = gpu_slam_factory(**mk), gpu_slam_factory(**mk)
    for s in (slam, plain):
        s.add_surf_point_cloud(sc.map_points)
    ids = [0, 1, 2]
    scans = [slam.host_alloc_like(_scan(sc, n, index=i)) for i in ids]
    pose0, deltas = sc.guess(0), chain_deltas(sc, ids)
    # A frame starts chained behind a registration that needs no more outer iterations than the one before it did (two, on a new
    # context): the run is made twice, the second time with the depth the first has learnt.  Every frame of both is compared.
    flags = []
    for call in range(2):
        res = slam.register_sequence(scans, pose0, deltas)
        _check_run(slam, plain, scans, pose0, deltas, res)
        flags += [st.flags for st in res[3]]
        print(pair, "call", call, "outer iterations", [st.n_iterations for st in res[3]], "flags", [hex(st.flags) for st in res[3]])
    assert all(bool(f & soicp.FLAG_QUERY_WAVES) == sed.takes_query_waves(n, msf) for f in flags), [hex(f) for f in flags]
    assert any(f & soicp.FLAG_CHAINED for f in flags), ("no frame started chained: the chained BEGIN launch did not run", [hex(f) for f in flags])
    keep = sed.keeps(n, msf)
    for s in (slam, plain):  # (both have registered the last frame last)
        ms = s.match_status(n)
        assert np.array_equal(ms == DROPPED, ~keep)
    assert np.array_equal(slam.match_status(n), plain.match_status(n))
    for st in res[3]:
        assert sum(st.iterations[0].reject_hist) == int(keep.sum())
    slam.close(); plain.close()


@pytest.mark.parametrize("pair", [(13734, 210), (1001, 1), (4097, 0)], ids=sed.pair_id)
def test_register_batch_hypotheses_equal_single_registrations(oracle, soicp, gpu_slam_factory, pair):
    """scan_keys_kernel<true>: three hypotheses, each the single registration from its guess to the bit -- also where no hypothesis has a query"""
    n, msf = pair
    sc = synth.Scene("small")
    slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=msf, max_iterations=5)
    slam.add_surf_point_cloud(sc.map_points)
    scan = _scan(sc, n)
    poses = np.stack([sc.guess(0), sc.guess(0, dt=0.2, dth_deg=2.0, seed_base=2000), sc.guess(0, dt=0.05, dth_deg=0.5, seed_base=3000)])
    d, _ = slam.upload_scan(scan)
    ok, rcs, out, sts = slam.register_batch(None, poses, d_scan=d, n=n)
    kept = int(sed.keeps(n, msf).sum())
    for h in range(3):
        rc, ph, sh = slam.register_dev(d, n, poses[h])
        assert rc == int(rcs[h]) == 0, (pair, h, rc, int(rcs[h]))
        assert np.array_equal(ph, out[h]), (pair, h)
        assert_same_bits(sts[h], sh, (pair, "batch against single", h), omit=("uncertainty",))  # (from the call before: the single ones advance it)
        assert sum(sts[h].iterations[0].reject_hist) == kept
    assert ok == 3
    slam.free_scan(d)
    slam.close()


@pytest.mark.parametrize("pair", [(13734, 210), (6401, 100)], ids=sed.pair_id)
@pytest.mark.parametrize("world_size", [2, 3])
def test_query_split_runs_the_rule_on_the_whole_scans_index(soicp, pair, world_size):
    """SO_ICP_SHARD_QUERIES: a rank holds the 64-point segments rank, rank + world, ... of a scan whose length is no multiple of 64 and
    applies the rule to the point's index in the WHOLE scan (scan_keys_kernel's gi)"""
    n, msf = pair
    assert n % 64 != 0
    sc = synth.Scene("small")
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=msf, max_iterations=5)
    one = soicp.LidarSlamGpu(**mk)
    one.add_surf_point_cloud(sc.map_points)
    ranks = [soicp.LidarSlamGpu(rank=r, world_size=world_size, shard_mode=soicp.SHARD_QUERIES, **mk) for r in range(world_size)]
    for sh in ranks:
        sh.comm_init_inprocess(0xB000 + 16 * world_size + (n % 16))
        assert sh.add_surf_point_cloud(sc.map_points) == len(sc.map_points)
    scan, guess = _scan(sc, n), sc.guess(0)
    kept = int(sed.keeps(n, msf).sum())
    ref = stats_of(one.register(scan, guess))
    res = in_threads(world_size, lambda r: stats_of(ranks[r].register(scan, guess)))
    for it in range(bits_field(ref[3], "n_iterations")):
        assert sum(bits_field(ref[3], "reject_hist", it)) == kept
    for r in range(world_size):
        assert res[r][1] == res[0][1], "all ranks hold the same sums"
        assert res[r][2] & soicp.FLAG_QUERY_SPLIT and res[r][2] & soicp.FLAG_SHARDED
        assert_rank_follows_single(res[r], ref, ("query split", pair, world_size, r))
        for it in range(bits_field(res[r][3], "n_iterations")):
            assert sum(bits_field(res[r][3], "reject_hist", it)) == kept, ("the histogram totals are the kept count of the WHOLE scan", r, it)
    for sh in ranks + [one]:
        sh.close()


# ------------------------------------------------------------------------------------------------------------------------
# bucket sizes of the binning
# ------------------------------------------------------------------------------------------------------------------------
PER_SIZE = 30


@pytest.fixture(scope="module")
def buckets(oracle, world):
    sc, fes, exp, om = world
    scan, owner = bed.bucket_scan(sc.map_points, sc.plane_res, per_size=PER_SIZE)
    sizes = bed.bucket_sizes(scan, sc.plane_res)
    assert np.array_equal(sizes, np.sort(np.repeat(np.array(bed.SIZES), PER_SIZE)))
    orc, _, ost, corrs = om.register(scan, IDENTITY, oracle.default_config(max_iterations=1), want_corrs=True)
    assert orc == 0
    return scan, bed.chunk_totals(sizes), ost, corrs


def _bucket_ctx(make, sc, env=None, **cfg):
    with _env(**(env or {})):
        slam = make(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=1, **cfg)
    slam.add_surf_point_cloud(sc.map_points)
    return slam


def _against_the_oracle(exp, scan, st, ms, nb, ost, corrs, tag):
    assert not (ms == DROPPED).any(), (tag, "a status byte of the registration before is left", np.nonzero(ms == DROPPED)[0][:8])
    assert np.array_equal(ms, corrs["status"]), (tag, "status bytes against the oracle", np.nonzero(ms != corrs["status"])[0][:8])
    judged = np.isin(corrs["status"], JUDGED)
    assert judged.sum() > len(scan) // 2
    _check_lists(exp, scan, ms, nb, judged, corrs["nbr"].reshape(-1, 5, 3), None, (tag, "oracle, query by query"))
    assert_follows_oracle(st, ost, tag)


@pytest.mark.parametrize("pack", ["1", "0"])
def test_bucket_sizes_around_the_cuts_of_bin_offsets(oracle, soicp, gpu_slam_factory, world, buckets, pack):
    sc, fes, exp, om = world
    scan, (normal, light), ost, corrs = buckets
    n = len(scan)
    # -- production: every status byte pre-set to 254 by (n, 0) registrations through so_icp_register_sequence's chained path (a
    #    registration swept by query waves there leaves the packing policy alone, where so_icp_register would note an empty work list
    #    that "fits": the registration behind it is the context's first chunked one and packs).  time_kernels 1 times the registration
    #    that starts with the count at a multiple of three: the counters are reset in front of it.
    slam = _bucket_ctx(gpu_slam_factory, sc, env={"SOICP_KNN_PACK": pack}, time_kernels=1)
    slam.set_max_surface_features(0)
    rc, _, _, sts, n_done = slam.register_sequence([scan, scan], IDENTITY, np.stack([IDENTITY, IDENTITY]))
    assert rc == 0 and n_done == 2 and all(s.flags & soicp.FLAG_QUERY_WAVES for s in sts), (rc, n_done, [hex(s.flags) for s in sts])
    assert (slam.match_status(n) == DROPPED).all()
    slam.set_max_surface_features(-1)
    slam.reset_timing()
    t0 = slam.timing()
    rc, _, st = slam.register(scan, IDENTITY)
    assert rc == 0 and not (st.flags & soicp.FLAG_QUERY_WAVES)
    ms, nb, t1 = slam.match_status(n), slam.neighbours(n), slam.timing()
    slam.close()
    packed = t1.knn_pack_registrations - t0.knn_pack_registrations
    print(f"pack={pack}: packed registrations {packed}, knn_queries {t1.knn_queries - t0.knn_queries}, chunks {normal} + {light} light")
    assert packed == (1 if pack == "1" else 0)
    assert (t1.knn_queries - t0.knn_queries, t1.knn_launches - t0.knn_launches) == (n, 1)
    _against_the_oracle(exp, scan, st, ms, nb, ost, corrs, ("buckets", pack))
    # -- the query-wave twin, in scans of at most 4 096 points
    qw = fes[0].slam
    qw.set_max_surface_features(-1); qw.set_max_iterations(1)
    j = np.isin(ms, JUDGED)
    for lo in range(0, n, 4096):
        part = np.ascontiguousarray(scan[lo:lo + 4096])
        rc, _, pst = qw.register(part, IDENTITY)
        assert rc == 0 and pst.flags & soicp.FLAG_QUERY_WAVES
        pms, pnb = qw.match_status(len(part)), qw.neighbours(len(part))
        assert np.array_equal(pms, ms[lo:lo + 4096]), (pack, lo, "status bytes against the query waves")
        assert np.array_equal(pnb[j[lo:lo + 4096]], nb[lo:lo + 4096][j[lo:lo + 4096]]), (pack, lo, "neighbour lists against the query waves")
    # -- the instrumented instantiation on a context of its own (its first registration: it packs where the switch allows): same bytes and
    #    lists, and one packed row per light chunk -- searched, or handed back for its x-runs or its tile
    prof = _bucket_ctx(gpu_slam_factory, sc, env={"SOICP_KNN_PACK": pack, "SOICP_ABLATE": ABLATE_STATS_ONLY}, time_kernels=2)
    rc, _, pst = prof.register(scan, IDENTITY)
    assert rc == 0
    pms, pnb, t = prof.match_status(n), prof.neighbours(n), prof.timing()
    prof.close()
    assert np.array_equal(pms, ms) and np.array_equal(pnb[j], nb[j]), (pack, "instrumented sweep")
    rows, handed_back = t.knn_packed_rows, t.knn_packed_rows_too_many_runs + t.knn_packed_rows_tile_full
    print(f"pack={pack} instrumented: packed registrations {t.knn_pack_registrations}, rows {t.knn_packed_rows} of them handed back "
          f"{t.knn_packed_rows_too_many_runs} + {t.knn_packed_rows_tile_full}, predicted light chunks {light}, knn_queries {t.knn_queries}")
    assert t.knn_queries == n and t.knn_launches == 1
    assert t.knn_pack_registrations == (1 if pack == "1" else 0)
    # knn_packed_rows counts a row once per PASS it has work in (knn_plane_kernel: `rows with work`, near and full pass alike), and
    # the two hand-back counters count rows that are in it already.  Every light chunk is a row of the near pass, and a row of the
    # full pass only where the near pass left one of its lanes uncertified: light <= rows <= 2 light.  (Measured on an MI355X with
    # 150 light chunks: 236 rows, none handed back.)  That no chunk is lost or doubled is held exactly by the 254 bytes, the
    # oracle's status bytes and lists for every query, and knn_queries above.
    if t.knn_pack_registrations:
        assert light <= rows <= 2 * light and handed_back <= rows, (pack, rows, handed_back, light)
    else:
        assert rows == 0 and handed_back == 0, (pack, rows, handed_back)


def test_bucket_sizes_with_the_scan_binned_ahead(oracle, soicp, gpu_slam_factory, world, buckets):
    """the same scan announced and binned ahead (bin_offsets_kernel adds to the slot's own counters).  Before every attempt a (n, 0)
    registration sets all status bytes to 254; the carrier's registration then rewrites the first CARRIER_N with statuses of OTHER queries."""
    sc, fes, exp, om = world
    scan, (normal, light), ost, corrs = buckets
    n = len(scan)
    slam = _bucket_ctx(gpu_slam_factory, sc)
    B = slam.host_alloc_like(scan)
    carrier, carrier_pose = slam.host_alloc_like(np.ascontiguousarray(sc.scan(1)[:CARRIER_N])), sc.guess(1)
    for attempt in range(16):
        slam.set_max_surface_features(0)
        rc, _, st0 = slam.register(scan, IDENTITY)
        assert rc == 0 and (slam.match_status(n) == DROPPED).all()
        slam.set_max_surface_features(-1)
        slam.stage_scan(B)
        slam.register(carrier, carrier_pose)
        rc, _, st = slam.register(B, IDENTITY)
        assert rc == 0 and st.flags & soicp.FLAG_STAGED_SCAN
        ms, nb = slam.match_status(n), slam.neighbours(n)
        _against_the_oracle(exp, scan, st, ms, nb, ost, corrs, ("buckets, staged", attempt))
        if st.flags & soicp.FLAG_BINNED_AHEAD:
            break
    slam.close()
    assert st.flags & soicp.FLAG_BINNED_AHEAD, "the scan was never binned ahead: the path was not exercised"


# ------------------------------------------------------------------------------------------------------------------------
# more than 2046 occupied cubes: the whole-cell key
# ------------------------------------------------------------------------------------------------------------------------
def test_whole_cell_key_of_a_map_with_more_than_2046_cubes(oracle, soicp, gpu_slam_factory):
    """scan_keys_kernel's cell_bits == 18.  Host-side map (no 16 MB pool region per cube), planeRes 1.0 (a cube's cell table is about
    90 kB): the small scene plus five points in each of 2 100 cubes outside every gate ball and outside the 5 x 5 x 3 block around the sensor.
    The registration is the one against the map without them, to the bit, and follows the oracle."""
    sc = synth.Scene("small")
    plane_res = 1.0
    far, cubes = bed.far_cube_points()
    scan, guess = sed.scan_of(sc, 5000, seed=77), sc.guess(0)
    res = {}
    with _env(SOICP_HOST_MAP="1"):
        for name, pts in (("plain", sc.map_points), ("far cubes", np.concatenate([sc.map_points, far]))):
            slam = gpu_slam_factory(plane_res=plane_res, line_res=plane_res / 2, max_surface_features=-1, max_iterations=5)
            slam.add_surf_point_cloud(pts)
            exp = slam.export_map()
            n_cubes = len(np.unique(ked.cube_of(exp), axis=0))
            out = []
            for max_it in (1, 5):
                slam.set_max_iterations(max_it)
                rc, pose, st = slam.register(scan, guess)
                assert rc == 0 and st.flags & soicp.FLAG_HOST_MAP and not (st.flags & soicp.FLAG_QUERY_WAVES), (name, rc, hex(st.flags))
                ms, nb = slam.match_status(len(scan)), slam.neighbours(len(scan))
                j = np.isin(ms, JUDGED)
                assert nb[j].max() < len(exp)
                out.append((st, pose, ms, exp[nb[j].astype(np.int64)]))  # (a host-side map: the indices are rows of export_map())
            res[name] = (exp, n_cubes, out)
            slam.close()
    exp, n_cubes, big = res["far cubes"]
    _, n_plain, plain = res["plain"]
    print("occupied cubes:", n_plain, "and", n_cubes)
    assert n_plain <= 64 and n_cubes == n_plain + len(cubes) > bed.KEY_SLOT_LIMIT
    om = oracle.OracleMap(plane_res=plane_res)
    assert om.add_surf(exp, raw=True) == len(exp)
    for k, max_it in enumerate((1, 5)):
        (st, pose, ms, nbr), (pst, ppose, pms, pnbr) = big[k], plain[k]
        tag = ("more than 2046 cubes", max_it)
        assert np.array_equal(ms, pms), (tag, "status bytes")
        assert np.array_equal(nbr.view(np.uint32), pnbr.view(np.uint32)), (tag, "neighbour coordinates")
        assert_same_bits(st, pst, tag)
        assert pose.tobytes() == ppose.tobytes()
        orc, opose, ost, corrs = om.register(scan, guess, oracle.default_config(max_iterations=max_it), want_corrs=True)
        assert orc == 0
        assert_follows_oracle(st, ost, tag, pose=pose, opose=opose)
        if max_it == 1:
            assert np.array_equal(ms, corrs["status"]), (tag, "status bytes against the oracle")
            j = np.isin(ms, JUDGED)
            assert j.sum() > 1000
            assert np.array_equal(nbr.view(np.uint32), corrs["nbr"].reshape(-1, 5, 3)[j].view(np.uint32)), (tag, "neighbours against the oracle")
