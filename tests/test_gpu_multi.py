"""-m gpu: N > 1 beyond the brick-hash shards of test_gpu_configs.py / test_gpu_peer.py.

  * SO_ICP_SHARD_QUERIES (map replicated on every rank, the scan's 64-point segments dealt round-robin, the same 45-double
    exchange per evaluation): ranks on ONE device, joined by an in-process group or by the peer exchange -- results equal to the
    single context (iteration counts, termination codes, histograms, accepted counts; poses to 1e-9) for even / odd world sizes,
    scan lengths that are not a multiple of 64, and with the max_surface_features sampling rule active;
  * the tests of the data plane ACROSS processes, the parent as control plane over pipes:
      - RCCL: ncclAllReduce of the 45 sums per evaluation (+ the map-count all-reduce of the insert) with both shard modes, and
        the RCCL all-gather re-cut of the shards at a planeRes change (so_icp_set_resolution under a communicator) -- one
        process per device; RCCL refuses two ranks on one device, so these skip unless so_icp_device_count() >= 2;
      - the peer exchange with hipIpcOpenMemHandle (tagged 16-byte chunks, over xGMI to ANOTHER device), both shard modes, and
        eight ranks: on a box with fewer GPUs than ranks the ranks share devices, and ranks of the same device share processes
        (helpers.rank_groups: at most MAX_RANK_PROCESSES rank processes where the device count allows it).
"""
import os
import sys

import numpy as np
import pytest

from helpers import MAX_RANK_PROCESSES, assert_rank_follows_single, bits_field, by_rank, in_threads, rank_groups, stats_of
from superodom_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((3, 0.4, 3.0), (9, 0.1, 1.0))  # (scan, guess dt, guess dtheta): the first needs several outer iterations


@pytest.mark.parametrize("world,n_keep,max_sf", [(2, None, -1), (3, 7001, -1), (4, 6000, 2500)])
def test_query_split_ranks_equal_the_single_context(soicp, world, n_keep, max_sf):
    """SO_ICP_SHARD_QUERIES with `world` contexts on this one GPU joined by an in-process group (per-evaluation launches, the sums
    through host memory): every rank registers its 64-point segments of the scan against the whole map."""
    sc = synth.Scene("small")
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=max_sf, max_iterations=5)
    one = soicp.LidarSlamGpu(**mk)
    one.add_surf_point_cloud(sc.map_points)
    ranks = [soicp.LidarSlamGpu(rank=r, world_size=world, shard_mode=soicp.SHARD_QUERIES, **mk) for r in range(world)]
    for sh in ranks:
        sh.comm_init_inprocess(0xA000 + world)
        assert sh.add_surf_point_cloud(sc.map_points) == len(sc.map_points)
        assert sh.map_size(this_rank=True) == (len(sc.map_points), len(sc.map_points)), "the map is replicated, not sharded"
    for i, dt, dth in CASES:
        scan = sc.scan(i)
        if n_keep:
            scan = np.ascontiguousarray(scan[:n_keep])
        guess = sc.guess(i, dt=dt, dth_deg=dth)
        ref = stats_of(one.register(scan, guess))
        if i == 3 and max_sf < 0:
            assert bits_field(ref[3], "n_iterations") >= 3, "the test needs several outer iterations"
        res = in_threads(world, lambda r: stats_of(ranks[r].register(scan, guess)))
        for r in range(world):
            assert res[r][1] == res[0][1], "all ranks hold the same sums: identical decisions, identical bits"
            assert res[r][2] & soicp.FLAG_QUERY_SPLIT and res[r][2] & soicp.FLAG_SHARDED
            assert_rank_follows_single(res[r], ref, ("query split", world, i, r))
    for sh in ranks + [one]:
        sh.close()


def test_query_split_over_the_peer_exchange_in_one_process(soicp, monkeypatch):
    """The same with the ranks' persistent solve launches trading their records through the inboxes (two contexts of one process,
    100 workgroups each so that both launches are co-resident on this one device)."""
    sc = synth.Scene("small")
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    one = soicp.LidarSlamGpu(**mk)
    one.add_surf_point_cloud(sc.map_points)
    monkeypatch.setenv("SOICP_SOLVE_WORKGROUPS", "100")
    ranks = [soicp.LidarSlamGpu(rank=r, world_size=2, shard_mode=soicp.SHARD_QUERIES, **mk) for r in range(2)]
    for sh in ranks:
        sh.add_surf_point_cloud(sc.map_points)
    handles = [sh.peer_export() for sh in ranks]
    assert in_threads(2, lambda r: ranks[r].peer_connect(handles)) == [True, True], [sh.last_error() for sh in ranks]
    for sh in ranks:
        sh.peer_enable(True)
    for i, dt, dth in CASES:
        scan, guess = sc.scan(i), sc.guess(i, dt=dt, dth_deg=dth)
        ref = stats_of(one.register(scan, guess))
        res = in_threads(2, lambda r: stats_of(ranks[r].register(scan, guess)))
        for r in range(2):
            assert res[r][1] == res[0][1]
            assert not (res[r][2] & soicp.FLAG_PER_EVAL_LAUNCHES), "the persistent solve launch must survive N > 1"
            assert_rank_follows_single(res[r], ref, ("query split, peer exchange", i, r))
    for sh in ranks + [one]:
        sh.close()


# ------------------------------------------------------------------------------------------------------------------------
# across processes: one device per rank where there are enough of them, otherwise the ranks share devices
# ------------------------------------------------------------------------------------------------------------------------
def _rank_process(ranks, world, shard_mode, transport, recut, conn):
    """One process = one or more ranks of ONE device (the peer exchange only: RCCL takes one rank per process and device), each
    driven from its own thread; the parent is the control plane over pipes."""
    try:
        sys.path.insert(0, ROOT)
        from superodom_amd import binding as soicp, synth as sy
        n_dev = soicp.device_count()
        if world > n_dev:  # ranks share a device: their persistent solve launches must be co-resident there (as bench.py sizes them)
            os.environ["SOICP_SOLVE_WORKGROUPS"] = str(max(16, 200 // ((world + n_dev - 1) // n_dev)))
        sc = sy.Scene("small")
        shs = [soicp.LidarSlamGpu(device_id=r % n_dev, plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1,
                                  max_iterations=5, rank=r, world_size=world, shard_mode=shard_mode) for r in ranks]
        if transport == "rccl" or recut:
            if ranks[0] == 0:
                conn.send(soicp.comm_unique_id())
            uid = conn.recv()
            shs[0].comm_init(uid)
        for sh in shs:
            sh.add_surf_point_cloud(sc.map_points)  # (collective under a communicator: the per-block counts of the full map)
        if transport == "peer":
            conn.send([sh.peer_export() for sh in shs])
            handles = conn.recv()  # all ranks' handles, rank order; same-process ones connect by pointer
            oks = in_threads(len(shs), lambda j: shs[j].peer_connect(handles))
            conn.send([(ok, sh.last_error()) for ok, sh in zip(oks, shs)])
            agreed = conn.recv()
            for sh in shs:
                sh.peer_enable(agreed)

        def register_all(out):
            for i, dt, dth in CASES:
                conn.recv()  # barrier
                scan, guess = sc.scan(i), sc.guess(i, dt=dt, dth_deg=dth)
                for j, res in enumerate(in_threads(len(shs), lambda j: shs[j].register(scan, guess))):
                    out[j].append(stats_of(res))
                conn.send(True)
        out = [[] for _ in shs]
        register_all(out)
        if recut:  # planeRes change over resident shards: the RCCL all-gather of every rank's owned points, then the same scans again
            conn.recv()
            shs[0].set_resolution(0.2, 0.4)
            out[0].append(("sizes", shs[0].map_size(this_rank=True)))
            register_all(out)
        conn.send(out)
        conn.recv()
        for sh in shs:
            sh.close()
    except BaseException as e:  # noqa: BLE001
        import traceback
        conn.send(("error", f"ranks {ranks}: {e!r}\n{traceback.format_exc()}"))
        raise


def _run_ranks(soicp, world, shard_mode, transport, recut=False):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    # RCCL: one rank per process and device.  Peer exchange: rank r on device r % n_dev; ranks share a process only on the same device
    groups = [[r] for r in range(world)] if (transport == "rccl" or recut) else rank_groups(world, soicp.device_count(), MAX_RANK_PROCESSES)
    n_procs = len(groups)
    pipes = [ctx.Pipe() for _ in range(n_procs)]
    procs = [ctx.Process(target=_rank_process, args=(groups[p], world, shard_mode, transport, recut, pipes[p][1])) for p in range(n_procs)]
    for p in procs:
        p.start()
    conns = [pp[0] for pp in pipes]

    def recv_all(which=None):
        out = []
        for c in (conns if which is None else [conns[k] for k in which]):
            assert c.poll(300), "a rank process did not answer"
            out.append(c.recv())
        errors = [o[1] for o in out if isinstance(o, tuple) and len(o) == 2 and o[0] == "error"]
        if errors:
            for p in procs:
                p.kill()
            pytest.fail("a rank process failed:\n" + "\n".join(errors))
        return out

    def send_all(v):
        for c in conns:
            c.send(v)
    if transport == "rccl" or recut:
        send_all(recv_all([0])[0])  # rank 0's unique id to everybody
    if transport == "peer":
        send_all(by_rank(groups, recv_all()))  # all handles, rank order
        oks = by_rank(groups, recv_all())
        agreed = all(o[0] for o in oks)
        send_all(agreed)
        assert agreed, f"hipIpc mapping / self-test failed: {oks}"
    n_rounds = len(CASES) * (2 if recut else 1)
    for k in range(n_rounds):
        if recut and k == len(CASES):
            send_all("recut")
        send_all("go")
        recv_all()
    res = by_rank(groups, recv_all())
    send_all("bye")
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return res


def _assert_same_over_map_shards(res, ref, k, tag):
    """Map shards joined by the peer exchange only: no communicator sums the per-block counts of the insert, so each rank reports
    the 5x5 count of ITS shard (laser_cloud_surf_from_map_num); the shards partition the map, so the counts add up to the single
    context's.  Everything else equals the single context rank by rank."""
    counts = [bits_field(r_[k][3], "laser_cloud_surf_from_map_num") for r_ in res]
    whole = bits_field(ref[k][3], "laser_cloud_surf_from_map_num")
    assert sum(counts) == whole and all(0 < c < whole for c in counts), (tag, counts, whole)
    for r, r_ in enumerate(res):
        assert_rank_follows_single(r_[k], ref[k], tag + (r,), omit=("laser_cloud_surf_from_map_num",))  # (compared as a sum, just above)


def _single_context_reference(soicp, plane_res=None):
    sc = synth.Scene("small")
    one = soicp.LidarSlamGpu(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    one.add_surf_point_cloud(sc.map_points)
    if plane_res:
        one.set_resolution(plane_res / 2, plane_res)
    out = [stats_of(one.register(sc.scan(i), sc.guess(i, dt=dt, dth_deg=dth))) for i, dt, dth in CASES]
    one.close()
    return out


def _need_devices(soicp, n):
    have = soicp.device_count()
    if have < n:
        pytest.skip(f"needs {n} HIP devices, this box has {have}: RCCL refuses two ranks on one device")


@pytest.mark.parametrize("shard_mode", [0, 1])
def test_rccl_two_ranks_on_two_devices_equal_the_single_context(soicp, shard_mode):
    _need_devices(soicp, 2)
    ref = _single_context_reference(soicp)
    res = _run_ranks(soicp, 2, shard_mode, "rccl")
    for k in range(len(CASES)):
        assert res[0][k][1] == res[1][k][1], "both ranks all-reduce the same sums: identical poses"
        for r in range(2):
            assert res[r][k][2] & soicp.FLAG_PER_EVAL_LAUNCHES, "RCCL path: one launch per evaluation"
            assert_rank_follows_single(res[r][k], ref[k], ("rccl", shard_mode, k, r))


@pytest.mark.parametrize("shard_mode", [0, 1])
def test_peer_exchange_across_two_devices_equals_the_single_context(soicp, shard_mode):
    """Two rank processes, inboxes mapped with hipIpcOpenMemHandle: over xGMI to the other device, or on the same one when the
    box has a single GPU."""
    ref = _single_context_reference(soicp)
    res = _run_ranks(soicp, 2, shard_mode, "peer")
    for k in range(len(CASES)):
        assert res[0][k][1] == res[1][k][1]
        for r in range(2):
            assert not (res[r][k][2] & soicp.FLAG_PER_EVAL_LAUNCHES), "the persistent solve launch must survive N > 1"
            if shard_mode == 1:  # (map replicated: every rank counts the whole map)
                assert_rank_follows_single(res[r][k], ref[k], ("peer over xGMI", shard_mode, k, r))
        if shard_mode == 0:
            _assert_same_over_map_shards(res, ref, k, ("peer over xGMI", shard_mode, k))


def test_rccl_all_gather_recuts_the_shards_at_a_plane_res_change(soicp):
    _need_devices(soicp, 2)
    ref_a = _single_context_reference(soicp)
    ref_b = _single_context_reference(soicp, plane_res=0.4)
    res = _run_ranks(soicp, 2, 0, "rccl", recut=True)
    n = len(CASES)
    for r in range(2):
        for k in range(n):
            assert_rank_follows_single(res[r][k], ref_a[k], ("before the re-cut", k, r))
        tag, sizes = res[r][n]
        assert tag == "sizes" and sizes[1] < sizes[0], "a shard, not the whole map, after the re-cut"
        for k in range(n):
            # (the ranks have registered these scans once before the re-cut, ref_b has not: another call before this one)
            assert_rank_follows_single(res[r][n + 1 + k], ref_b[k], ("after the re-cut", k, r), omit=("uncertainty",))


def test_eight_ranks_on_eight_devices(soicp):
    """The bench's N = 8 configuration in miniature: peer exchange, brick-hash shards (ranks share devices and processes where
    the box has fewer than eight GPUs)."""
    ref = _single_context_reference(soicp)
    res = _run_ranks(soicp, 8, 0, "peer")
    for k in range(len(CASES)):
        for r in range(8):
            assert res[r][k][1] == res[0][k][1]
        _assert_same_over_map_shards(res, ref, k, ("8 ranks", k))
