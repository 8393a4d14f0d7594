"""-m gpu: the peer exchange (so_icp_peer_export / _connect / _enable) -- the ranks' persistent solve launches trade their
records through inboxes mapped into each other's address space instead of a collective per evaluation.  Both ranks sit on
this box's single GPU (RCCL refuses two ranks on one device; IPC handles and same-process pointers do not), each with
SOICP_SOLVE_WORKGROUPS=100 so that the two persistent launches are co-resident:
  * two shard contexts of ONE process, each driven from its own thread (inboxes connected by pointer);
  * rank PROCESSES (multiprocessing spawn; the parent is the control plane that carries the handles and the agreement over pipes),
    inboxes mapped with hipIpcOpenMemHandle -- the path bench.py takes for --gpus N; at most MAX_RANK_PROCESSES of them hold the
    GPU at once (tests/helpers.py), so N = 8 puts two ranks (one thread each, connected by pointer) in every process.
Results must equal the single-context registration: iteration counts, termination codes, histograms; poses to 1e-9."""
import os
import sys

import numpy as np
import pytest

from helpers import MAX_RANK_PROCESSES, assert_rank_follows_single, bits_field, by_rank, in_threads, rank_groups, stats_of
from superodom_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((3, 0.4, 3.0), (9, 0.1, 1.0), (14, 0.1, 1.0))  # (scan, guess dt, guess dtheta): the first needs several outer iterations


def _reference(soicp, sc):
    one = soicp.LidarSlamGpu(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    one.add_surf_point_cloud(sc.map_points)
    out = [stats_of(one.register(sc.scan(i), sc.guess(i, dt=dt, dth_deg=dth))) for i, dt, dth in CASES]
    one.close()
    return out


@pytest.mark.parametrize("world,wgs", [(2, 100)])
def test_peer_exchange_between_contexts_of_one_process(soicp, monkeypatch, world, wgs):
    """Two shard contexts on this one GPU (2 x 100 <= 256 compute units, so that both persistent solve launches are
    co-resident), each driven from its own thread; the map-count collective of the inserts goes through an in-process group.
    (More ranks than that belong in separate processes -- the next test: the streams of ONE process share its hardware
    queues, GPU_MAX_HW_QUEUES = 4 by default, and two solve launches on one queue cannot run at the same time.)"""
    sc = synth.Scene("small")
    ref = _reference(soicp, sc)
    assert bits_field(ref[0][3], "n_iterations") >= 3
    monkeypatch.setenv("SOICP_SOLVE_WORKGROUPS", str(wgs))
    ranks = list(range(world))
    shards = [soicp.LidarSlamGpu(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5,
                                 rank=r, world_size=world) for r in ranks]
    for sh in shards:
        sh.comm_init_inprocess(0x9000 + world)
    in_threads(world, lambda r: shards[r].add_surf_point_cloud(sc.map_points) or True, 180)  # collective: the full-map counts are summed
    sizes = [sh.map_size(this_rank=True) for sh in shards]
    assert all(t == len(sc.map_points) and m < t for t, m in sizes)
    handles = [sh.peer_export() for sh in shards]
    oks = in_threads(world, lambda r: shards[r].peer_connect(handles), 180)
    assert oks == [True] * world, [sh.last_error() for sh in shards]
    for sh in shards:
        sh.peer_enable(True)
    for k, (i, dt, dth) in enumerate(CASES):
        scan, guess = sc.scan(i), sc.guess(i, dt=dt, dth_deg=dth)
        res = in_threads(world, lambda r: shards[r].register(scan, guess), 180)
        for r in ranks:
            assert np.array_equal(res[r][1], res[0][1]), "all ranks hold the same sums: identical decisions, identical bits"
            assert_rank_follows_single(stats_of(res[r]), ref[k], ("in-process", world, i, r))
            assert not (res[r][2].flags & soicp.FLAG_PER_EVAL_LAUNCHES), "the persistent solve launch must survive N > 1"


def _peer_worker(ranks, world, wgs, conn):
    """One process = one or more ranks, each driven from its own thread.  The parent is the control plane (it carries the
    handles, the agreement and the barriers over pipes -- any transport will do, bench.py uses gloo).  An exception travels
    to the parent as ("error", text), so that the test fails at once instead of waiting for an answer that will not come."""
    try:
        _peer_worker_body(ranks, world, wgs, conn)
    except BaseException as e:  # noqa: BLE001
        import traceback
        conn.send(("error", f"ranks {ranks}: {e!r}\n{traceback.format_exc()}"))
        raise


def _peer_worker_body(ranks, world, wgs, conn):
    sys.path.insert(0, ROOT)
    os.environ["SOICP_SOLVE_WORKGROUPS"] = str(wgs)
    from superodom_amd import binding as soicp, synth as sy
    sc = sy.Scene("small")
    shards = [soicp.LidarSlamGpu(device_id=0, plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5,
                                 rank=r, world_size=world) for r in ranks]
    for sh in shards:
        sh.add_surf_point_cloud(sc.map_points)
    conn.send([sh.peer_export() for sh in shards])
    handles = conn.recv()                 # all ranks' handles, rank order (doubles as a barrier); same-process ones connect by pointer
    oks = in_threads(len(shards), lambda j: shards[j].peer_connect(handles))
    conn.send([(ok, sh.last_error()) for ok, sh in zip(oks, shards)])
    agreed = conn.recv()
    for sh in shards:
        sh.peer_enable(agreed)
    out = [[] for _ in shards]
    for i, dt, dth in CASES:
        conn.recv()                       # barrier: all ranks start the registration together
        scan, guess = sc.scan(i), sc.guess(i, dt=dt, dth_deg=dth)
        res = in_threads(len(shards), lambda j: shards[j].register(scan, guess))
        for j, (rc, pose, st) in enumerate(res):
            out[j].append(stats_of((rc, pose, st)))
        conn.send(True)
    conn.send(out)
    conn.recv()
    for sh in shards:
        sh.close()


@pytest.mark.parametrize("world,wgs", [(2, 100), (4, 60), (8, 30)])
def test_peer_exchange_between_processes_over_hip_ipc(soicp, world, wgs):
    """N = 2, 4, 8 ranks on this one GPU (N x wgs <= 256 compute units) in at most MAX_RANK_PROCESSES processes, inboxes
    mapped with hipIpcOpenMemHandle between processes (N = 8: two ranks per process, connected by pointer inside it)."""
    import multiprocessing as mp
    sc = synth.Scene("small")
    ref = _reference(soicp, sc)
    ctx = mp.get_context("spawn")
    groups = rank_groups(world, 1, MAX_RANK_PROCESSES)  # (every rank on device 0)
    n_procs = len(groups)
    pipes = [ctx.Pipe() for _ in range(n_procs)]
    procs = [ctx.Process(target=_peer_worker, args=(groups[p], world, wgs, pipes[p][1])) for p in range(n_procs)]
    for p in procs:
        p.start()
    conns = [pp[0] for pp in pipes]

    def recv_all():
        out = []
        for c in conns:
            assert c.poll(240), "a rank process did not answer"
            out.append(c.recv())
        errors = [o[1] for o in out if isinstance(o, tuple) and len(o) == 2 and o[0] == "error"]
        if errors:
            for p in procs:
                p.kill()
            pytest.fail("a rank process failed:\n" + "\n".join(errors))
        return out
    handles = by_rank(groups, recv_all())
    for c in conns:
        c.send(handles)
    oks = by_rank(groups, recv_all())
    agreed = all(o[0] for o in oks)
    for c in conns:
        c.send(agreed)
    assert agreed, f"hipIpc mapping / self-test failed: {oks}"
    for _ in CASES:
        for c in conns:
            c.send("go")
        recv_all()
    res = by_rank(groups, recv_all())
    for c in conns:
        c.send("bye")
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for k, (i, dt, dth) in enumerate(CASES):
        a = res[0][k]
        for r in range(1, world):
            assert res[r][k][0] == a[0] == 0 and res[r][k][1] == a[1], "all processes must return identical poses"
        assert not (a[2] & soicp.FLAG_PER_EVAL_LAUNCHES)
        # (no communicator between the processes: each rank counts the map points of its own shard; test_gpu_multi.py adds them up)
        assert_rank_follows_single(a, ref[k], ("processes", world, i), omit=("laser_cloud_surf_from_map_num",))
