"""-m gpu: so_icp_localization_sequence -- a run of frames in the reference's per-frame order (LidarSlam.cpp:30-51, 107-167): register
frame k from guess_k = pose_out_(k-1) o delta_k, then insert it into the map, then the next frame.  Required: every frame is THE
so_icp_localization call a per-frame loop makes from guesses_out[k] -- poses, statistics and the map after the run identical bit for bit
(also after a partial run) --, guesses_out chains from pose_out (after MannualYawCorrection), resident scans give the same bits, a run
that crosses a 50 m block boundary into a cube the map did not have and a guess that leaves its block stay bit-equal, a frame without
enough map stops the run there like the loop does, and the oracle's register + transform_and_add loop agrees from the same guesses."""
import os

import numpy as np
import pytest

from helpers import assert_follows_oracle, assert_same_bits, chain_deltas, scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu


def _contexts(factory, sc, n=2, **kw):
    out = [scene_with_oracle(sc, None, factory, oracle_too=False, **dict(dict(max_iterations=5), **kw))[1] for _ in range(n)]
    for s in out:
        s.shift_map(sc.gt_pose(0)[:3])
    return out


def _per_frame(plain, scans, guesses, times):
    """the loop a caller runs today: so_icp_localization per frame from the guesses the run reported"""
    poses, stats = [], []
    for k in range(len(scans)):
        rc, pose, st = plain.localization(True, guesses[k], scans[k], times[k])
        if rc != 0:
            return rc, k, np.array(poses).reshape(-1, 7), stats
        poses.append(pose); stats.append(st)
    return 0, len(scans), np.array(poses).reshape(-1, 7), stats


def _assert_maps_equal(a, b, pos):
    assert a.map_size() == b.map_size()
    ra, rb = a.export_map_records(stride=12), b.export_map_records(stride=12)
    assert ra.shape == rb.shape and ra.tobytes() == rb.tobytes(), "maps differ"
    assert a.count_5x5(pos) == b.count_5x5(pos)


def _assert_run_matches(res, ref, pose0, deltas):
    rc, poses, guesses, stats, n_done = res
    rrc, rn, rposes, rstats = ref
    assert rc == rrc and n_done == rn, (rc, rrc, n_done, rn)
    assert np.array_equal(guesses[0], np.asarray(pose0, float))
    for k in range(1, n_done):  # the chain continues from pose_out (after MannualYawCorrection), composed on the host
        assert np.array_equal(guesses[k], synth.pose_compose(poses[k - 1], deltas[k])), k
    assert np.array_equal(poses[:n_done], rposes), "poses differ from the per-frame loop"
    for k in range(n_done):
        assert_same_bits(stats[k], rstats[k], ("frame", k))


@pytest.mark.parametrize("scene,n_frames,pinned", [("small", 9, True), ("tiny", 9, False), ("os1_128_2m", 8, True)])
def test_sequence_equals_the_per_frame_loop_including_the_map(gpu_slam_factory, scene, n_frames, pinned):
    sc = synth.Scene(scene)
    seq, plain = _contexts(gpu_slam_factory, sc)
    ids = list(range(n_frames))
    host = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in ids]
    scans = [seq.host_alloc_like(h) for h in host] if pinned else host
    deltas = chain_deltas(sc, ids); times = 0.1 * np.arange(1, n_frames + 1)
    pose0 = sc.guess(0)
    # a partial run of 3 frames first: an insert applied late or twice shows in the map here
    res3 = seq.localization_sequence(scans[:3], pose0, deltas[:3], times[:3])
    ref3 = _per_frame(plain, host[:3], res3[2], times[:3])
    _assert_run_matches(res3, ref3, pose0, deltas[:3])
    _assert_maps_equal(seq, plain, res3[3][2].pos_in_localmap)
    # the rest of the run, chained on from the last pose of the first call
    pose0b = synth.pose_compose(res3[1][2], deltas[3])
    rest_deltas = deltas[3:].copy(); rest_deltas[0] = [0, 0, 0, 0, 0, 0, 1.0]
    res = seq.localization_sequence(scans[3:], pose0b, rest_deltas, times[3:])
    ref = _per_frame(plain, host[3:], res[2], times[3:])
    _assert_run_matches(res, ref, pose0b, rest_deltas)
    assert res[0] == 0 and res[4] == n_frames - 3, seq.last_error()
    _assert_maps_equal(seq, plain, res[3][-1].pos_in_localmap)
    assert seq.map_size() > 0
    # the registrations still land on the trajectory
    for k, i in enumerate(ids[3:]):
        dt, dr = synth.pose_error(res[1][k], sc.gt_pose(i))
        assert dt < 0.05 and dr < 0.01, (i, dt, dr)
    seq.close(); plain.close()


def test_off_by_metres_prediction_and_resident_scans_give_the_same_bits(gpu_slam_factory, soicp):
    """a frame predicted 1.5 m off (more outer iterations); the same run from resident scans on a fresh context -- all the loop's bits"""
    sc = synth.Scene("small")
    seq, plain = _contexts(gpu_slam_factory, sc)
    ids = list(range(8))
    host = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in ids]
    scans = [seq.host_alloc_like(h) for h in host]
    deltas = chain_deltas(sc, ids, x_off={4: 1.5}); times = 0.1 * np.arange(1, 9)
    pose0 = sc.guess(0)
    res = seq.localization_sequence(scans, pose0, deltas, times)
    ref = _per_frame(plain, host, res[2], times)
    _assert_run_matches(res, ref, pose0, deltas)
    assert res[0] == 0
    print("outer iterations per frame", [st.n_iterations for st in res[3]])
    _assert_maps_equal(seq, plain, res[3][-1].pos_in_localmap)

    (resident,) = _contexts(gpu_slam_factory, sc, n=1)
    d_scans = [resident.upload_scan(h) for h in host]
    res_d = resident.localization_sequence(d_scans, pose0, deltas, times, on_device=True)
    assert res_d[0] == 0
    assert np.array_equal(res_d[1], res[1]) and np.array_equal(res_d[2], res[2])
    for k, (a, b) in enumerate(zip(res_d[3], res[3])):
        assert_same_bits(a, b, ("resident scans, frame", k))
    _assert_maps_equal(resident, seq, res[3][-1].pos_in_localmap)
    for s in (seq, plain, resident):
        s.close()


def test_a_run_across_a_block_boundary_into_a_new_cube(gpu_slam_factory):
    """The world moved +28.9 m in x: the trajectory starts at x = 24.4 and crosses the 50 m block boundary at x = 25 (LocalMap.h:488-497)
    around frame 4; the seeded map is cut at that boundary, so the inserts open a cube it did not have.  The last frame's prediction is
    30 m off, its guess in another block than the frame before.  Poses, statistics and the map stay the per-frame loop's."""
    sc = synth.Scene("small")
    off = np.array([28.9, 0.0, 0.0])
    world_map = sc.map_points + off.astype(np.float32)
    world_map = np.ascontiguousarray(world_map[world_map[:, 0] < 25.0])
    mk = dict(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=5)
    seq, plain = gpu_slam_factory(**mk), gpu_slam_factory(**mk)
    for s_ in (seq, plain):
        s_.add_surf_point_cloud(world_map)
        s_.shift_map(sc.gt_pose(0)[:3] + off)
    assert not (seq.export_map()[:, 0] >= 25.0).any()
    ids = list(range(10))
    host = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in ids]
    deltas = chain_deltas(sc, ids, x_off={9: -30.0}); times = 0.1 * np.arange(1, 11)
    pose0 = sc.guess(0).copy(); pose0[:3] += off
    res = seq.localization_sequence([seq.host_alloc_like(h) for h in host], pose0, deltas, times)
    assert res[0] == 0 and res[4] == len(ids), (res[0], res[4], seq.last_error())
    ref = _per_frame(plain, host, res[2], times)
    _assert_run_matches(res, ref, pose0, deltas)
    _assert_maps_equal(seq, plain, res[3][-1].pos_in_localmap)
    xs = [st.pos_in_localmap[0] for st in res[3]]
    print("block x per frame", xs, "guess x", [round(g[0], 2) for g in res[2]])
    assert xs[0] == 10 and 11 in xs[:9], xs                      # the window's block followed the trajectory across the boundary
    assert xs[9] != xs[8], xs                                    # the off-by-metres guess left the block of the frame before it
    assert (seq.export_map()[:, 0] >= 25.0).any()                # the inserts opened the cube beyond the boundary
    seq.close(); plain.close()


def test_a_frame_without_map_stops_the_run_like_the_loop(gpu_slam_factory, soicp):
    """frame 3 is predicted 250 m away, where the 5x5 window holds no map: SO_ICP_NOT_ENOUGH_MAP_FEATURES, n_done 3, the map holds
    exactly the three frames before it, and the context goes on working"""
    sc = synth.Scene("small")
    seq, plain = _contexts(gpu_slam_factory, sc)
    ids = list(range(6))
    host = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in ids]
    deltas = chain_deltas(sc, ids, x_off={3: 250.0}); times = 0.1 * np.arange(1, 7)
    pose0 = sc.guess(0)
    res = seq.localization_sequence(host, pose0, deltas, times)
    assert res[0] == soicp.NOT_ENOUGH_MAP_FEATURES and res[4] == 3, (res[0], res[4], seq.last_error())
    ref = _per_frame(plain, host, res[2], times)
    assert ref[0] == soicp.NOT_ENOUGH_MAP_FEATURES and ref[1] == 3
    _assert_run_matches(res, ref, pose0, deltas)
    _assert_maps_equal(seq, plain, res[3][2].pos_in_localmap)
    # the next call on either context works and agrees
    a = seq.localization(True, sc.guess(4), host[4], 0.55)
    b = plain.localization(True, sc.guess(4), host[4], 0.55)
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1])
    _assert_maps_equal(seq, plain, a[2].pos_in_localmap)
    seq.close(); plain.close()


def test_the_oracle_agrees_from_the_same_guesses(oracle, gpu_slam_factory):
    sc = synth.Scene("small")
    (seq,) = _contexts(gpu_slam_factory, sc, n=1)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(seq.export_map(), raw=True)
    om.shift(sc.gt_pose(0)[:3])
    cfg = oracle.default_config(max_iterations=5)
    ids = list(range(8))
    host = [np.ascontiguousarray(sc.scan(i), dtype=np.float32) for i in ids]
    deltas = chain_deltas(sc, ids); times = 0.1 * np.arange(1, 9)
    res = seq.localization_sequence([seq.host_alloc_like(h) for h in host], sc.guess(0), deltas, times)
    assert res[0] == 0 and res[4] == len(ids)
    prev_hist = None
    for k in range(len(ids)):
        orc, opose, ost, _ = om.register(host[k], res[2][k], cfg, prev_obs_hist=prev_hist)
        st = res[3][k]
        assert orc == 0, k
        assert_follows_oracle(st, ost, ("frame", k), pose=res[1][k], opose=opose)
        prev_hist = np.array(ost.iters[ost.n_iterations - 1].obs_hist, np.int32)
        om.transform_and_add(host[k], res[1][k])  # the oracle's map follows the product's poses
    assert seq.map_size() == om.size(), "the inserts of the run differ from the oracle's VoxelGrid insert"
    a = seq.export_map(); b = om.export()
    assert np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])
    seq.close()


def test_the_cpp_adapter_replays_a_run_through_the_sequence(gpu_slam_factory, tmp_path):
    """adapter/adapter_driver --sequence: LidarSLAM::LocalizationSequence after a seeding frame, pcl::PointXYZI clouds (stride 32);
    its poses are the Python-driven sequence's up to the rounding of the motion predictions (composed in C++ there, in numpy here)"""
    import struct
    import subprocess
    driver = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adapter", "adapter_driver")
    assert os.path.exists(driver), "adapter/adapter_driver not built: run python __graft_entry__.py"
    sc = synth.Scene("tiny")
    n_frames, max_it = 7, 4
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in range(n_frames)]
    guesses = [sc.gt_pose(0)] + [sc.guess(i) for i in range(1, n_frames)]
    times = [0.1 * i for i in range(n_frames)]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ifii", n_frames, sc.plane_res, max_it, -1))
        for i in range(n_frames):
            f.write(struct.pack("<i", len(scans[i])))
            f.write(np.asarray(guesses[i], np.float64).tobytes()); f.write(struct.pack("<d", times[i])); f.write(scans[i].tobytes())
    r = subprocess.run([driver, str(fin), str(fout), "--sequence"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    raw = open(fout, "rb").read()
    status, n_done = struct.unpack_from("<ii", raw, 0)
    assert status == 0 and n_done == n_frames - 1, (status, n_done)
    cpp_poses = np.frombuffer(raw, np.float64, 7 * n_done, 8).reshape(-1, 7)
    printed = np.array([[float(v) for v in line.split(":")[1].split()] for line in r.stdout.splitlines() if line.startswith("frame")])
    assert np.array_equal(printed, cpp_poses)

    slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=max_it)
    assert slam.localization(False, guesses[0], scans[0], times[0])[0] == 2
    deltas = np.zeros((n_frames - 1, 7)); deltas[:, 6] = 1.0
    for k in range(1, n_frames - 1):
        deltas[k] = synth.pose_between(guesses[k], guesses[k + 1])
    res = slam.localization_sequence(scans[1:], guesses[1], deltas, times[1:])
    assert res[0] == 0 and res[4] == n_frames - 1
    for k in range(n_done):
        dt, dr = synth.pose_error(cpp_poses[k], res[1][k])
        assert dt < 1e-6 and dr < 1e-6, (k, dt, dr)
    slam.close()
