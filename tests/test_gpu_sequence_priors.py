"""-m gpu: so_icp_set_sequence_priors -- one pose prior per frame of a run, measured where the caller says or at the frame's own guess,
the run staying chained.  The contract: with P_k = priors[k] (AT_GUESS: T_meas := guesses_out[k]), frame k of so_icp_register_sequence
is so_icp_set_pose_prior(P_k) + so_icp_register from guesses_out[k] bit for bit -- on the chained path (where a chained AT_GUESS frame
runs solve_kernel_prior_at_guess, T_meas read from DevState::pose_in), from resident scans, unchained, and across a broken chain --, and
frame k of so_icp_localization_sequence that call + so_icp_localization, the map after every frame included.  Scenes and sizes are
those of test_gpu_sequence.py; tests/test_sequence_priors_host.py shows on the CPU that the priors used here make the runs take the
paths the conditions below name."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_prior_ref as ppr
import sequence_priors_data as spd
from helpers import CARRIED_OVER_FIELDS, assert_same_bits, scene_with_oracle
from superodom_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "adapter", "adapter_driver")
IU = np.triu_indices(6)
CHAINED_RUNS = ("small_chunked", "small_sampled", "tiny")


def _make(factory, run, **extra):
    r = spd.RUNS[run]
    sc = synth.Scene(r["scene"])
    slam = factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=r["max_feat"], max_iterations=spd.MAX_OUTER, **extra)
    slam.add_surf_point_cloud(sc.map_points)
    return slam


def _check_contract(soicp, twin, scans, pose0, deltas, priors, modes, res, tag):
    """every frame of the run against so_icp_set_pose_prior(P_k) + so_icp_register from guesses_out[k] on a twin context"""
    rc, poses, guesses, stats, n_done = res
    assert rc == 0 and n_done == len(scans), (tag, rc, n_done)
    assert np.array_equal(guesses[0], np.asarray(pose0, float))
    for k in range(len(scans)):
        if k:
            last = stats[k - 1].iterations[stats[k - 1].n_iterations - 1]
            want = synth.pose_compose(np.array(last.pose_after), deltas[k])
            assert np.array_equal(guesses[k], want), (tag, k, guesses[k] - want)  # the device's composition == the host's, bit for bit
        P = spd.frame_prior(priors, modes, k, guesses[k])
        if P is not None:
            twin.set_pose_prior(P)
        prc, ppose, pst = twin.register(scans[k], guesses[k])
        assert prc == 0
        assert np.array_equal(ppose, poses[k]), (tag, k, modes[k], ppose - poses[k])
        assert_same_bits(pst, stats[k], (tag, "frame", k, "mode", modes[k]))
        has = P is not None
        assert bool(stats[k].flags & soicp.FLAG_POSE_PRIOR) == has == bool(pst.flags & soicp.FLAG_POSE_PRIOR), (tag, k, hex(stats[k].flags))
        assert stats[k].prediction_source == pst.prediction_source == (1 if has else 0), (tag, k)


_runs = {}


@pytest.fixture(scope="module")
def chained_run(soicp, gpu_slam_factory):
    """(run, kind) -> the run on a fresh context, chained, from pinned host scans, and that context (later tests run it again on it)"""
    def get(run, kind):
        if (run, kind) not in _runs:
            sc, scans, pose0, deltas, priors, modes = spd.run_inputs(run, kind)
            slam = _make(gpu_slam_factory, run)
            pinned = [slam.host_alloc_like(s) for s in scans]
            slam.set_sequence_priors(priors, modes)
            res = slam.register_sequence(pinned, pose0, deltas)
            _runs[(run, kind)] = (slam, pinned, pose0, deltas, priors, modes, res, slam.timing())
        return _runs[(run, kind)]
    yield get
    for entry in _runs.values():
        entry[0].close()
    _runs.clear()


# ---- 1. the run equals the per-frame calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", spd.U_KINDS)
@pytest.mark.parametrize("run", CHAINED_RUNS)
def test_run_equals_the_per_frame_calls(soicp, gpu_slam_factory, chained_run, run, kind):
    slam, scans, pose0, deltas, priors, modes, res, timing = chained_run(run, kind)
    twin = _make(gpu_slam_factory, run)
    _check_contract(soicp, twin, scans, pose0, deltas, priors, modes, res, f"{run} {kind}")
    twin.close()
    flags = [st.flags for st in res[3]]
    chained = [bool(f & soicp.FLAG_CHAINED) for f in flags]
    print(run, kind, "outer iterations", [st.n_iterations for st in res[3]], "modes", modes, "chained", chained, "chain breaks", timing.seq_chain_breaks)
    qw = spd.RUNS[run]["scene"] == "tiny" or spd.RUNS[run]["max_feat"] == 3000
    assert all(bool(f & soicp.FLAG_QUERY_WAVES) == qw for f in flags), [hex(f) for f in flags]
    # what makes solve_kernel_prior_at_guess run: a CHAINED frame whose prior is measured at its guess
    assert timing.seq_chained >= 2 and sum(chained) >= 2, chained
    assert any(c and m == spd.AT_GUESS for c, m in zip(chained, modes)), (chained, modes)
    assert sorted(set(modes)) == [spd.NONE, spd.GIVEN, spd.AT_GUESS]


# ---- 2. the same run on the other paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", spd.U_KINDS)
@pytest.mark.parametrize("run", CHAINED_RUNS)
def test_resident_scans_and_the_unchained_path_give_the_same_bits(soicp, gpu_slam_factory, monkeypatch, chained_run, run, kind):
    slam, scans, pose0, deltas, priors, modes, res, _ = chained_run(run, kind)
    d_scans = [slam.upload_scan(s) for s in scans]
    slam.set_sequence_priors(priors, modes)
    res_dev = slam.register_sequence(d_scans, pose0, deltas, on_device=True)
    assert res_dev[0] == 0 and np.array_equal(res_dev[1], res[1]) and np.array_equal(res_dev[2], res[2])
    for k, (a, b) in enumerate(zip(res_dev[3], res[3])):
        assert_same_bits(a, b, (run, kind, "resident scans", k), omit=CARRIED_OVER_FIELDS)  # (carried over from the call before)
        assert (a.flags & soicp.FLAG_POSE_PRIOR) == (b.flags & soicp.FLAG_POSE_PRIOR) and a.prediction_source == b.prediction_source
    monkeypatch.setenv("SOICP_SEQ_CHAIN", "0")  # (read when the context is made)
    unchained = _make(gpu_slam_factory, run)
    unchained.set_sequence_priors(priors, modes)
    res_u = unchained.register_sequence(scans, pose0, deltas)
    unchained.close()
    assert res_u[0] == 0 and np.array_equal(res_u[1], res[1]) and np.array_equal(res_u[2], res[2])
    for k, (a, b) in enumerate(zip(res_u[3], res[3])):
        assert_same_bits(a, b, (run, kind, "unchained", k))
        assert (a.flags & soicp.FLAG_POSE_PRIOR) == (b.flags & soicp.FLAG_POSE_PRIOR) and a.prediction_source == b.prediction_source
    assert not any(st.flags & soicp.FLAG_CHAINED for st in res_u[3])


# ---- 3. across a broken chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", spd.U_KINDS)
def test_a_broken_chain_keeps_the_contract(soicp, gpu_slam_factory, chained_run, kind):
    slam, scans, pose0, deltas, priors, modes, res, timing = chained_run("broken", kind)
    assert modes == [spd.AT_GUESS] * len(scans)
    twin = _make(gpu_slam_factory, "broken")
    _check_contract(soicp, twin, scans, pose0, deltas, priors, modes, res, f"broken {kind}")
    twin.close()
    iters = [st.n_iterations for st in res[3]]
    print("broken", kind, "outer iterations", iters, "| chained", timing.seq_chained, "| chain breaks", timing.seq_chain_breaks, "| flags", [hex(st.flags) for st in res[3]])
    assert max(iters) > min(iters), iters
    assert timing.seq_chain_breaks >= 1, (iters, timing.seq_chain_breaks)
    assert timing.seq_chained >= 1


# ---- 4. all NONE ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["small_chunked", "tiny"])
def test_all_none_is_the_run_without_priors(soicp, gpu_slam_factory, run):
    sc, scans, pose0, deltas, priors, _ = spd.run_inputs(run, "dense")
    results = []
    for with_call in (False, True):
        slam = _make(gpu_slam_factory, run)
        pinned = [slam.host_alloc_like(s) for s in scans]
        if with_call:
            slam.set_sequence_priors(priors, [spd.NONE] * len(scans))
        results.append(slam.register_sequence(pinned, pose0, deltas))
        slam.close()
    plain, none = results
    assert plain[0] == none[0] == 0
    assert plain[1].tobytes() == none[1].tobytes() and plain[2].tobytes() == none[2].tobytes()
    for k, (a, b) in enumerate(zip(none[3], plain[3])):
        assert_same_bits(a, b, (run, "all NONE", k))
        assert a.flags == b.flags and not (a.flags & soicp.FLAG_POSE_PRIOR) and a.prediction_source == b.prediction_source == 0, (k, hex(a.flags), hex(b.flags))


# ---- 5. U = 0 at the guess ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["small_chunked", "tiny"])
def test_nothing_to_add_at_the_guess(soicp, gpu_slam_factory, run):
    sc, scans, pose0, deltas, _, _ = spd.run_inputs(run, "dense")
    zero = soicp.pose_prior(np.full(7, np.nan), np.zeros((6, 6)), ppr.REFERENCE_FLOOR, ppr.REFERENCE_FRACTION)
    results = []
    for with_priors in (False, True):
        slam = _make(gpu_slam_factory, run)
        pinned = [slam.host_alloc_like(s) for s in scans]
        if with_priors:
            slam.set_sequence_priors([zero] * len(scans), [spd.AT_GUESS] * len(scans))
        results.append((slam.register_sequence(pinned, pose0, deltas), slam.timing().seq_chained))
        slam.close()
    (plain, plain_chained), (res, res_chained) = results
    assert plain[0] == res[0] == 0
    assert plain[1].tobytes() == res[1].tobytes() and plain[2].tobytes() == res[2].tobytes()
    for k, (a, b) in enumerate(zip(res[3], plain[3])):
        assert_same_bits(a, b, (run, "U = 0", k))
        assert a.flags == b.flags | soicp.FLAG_POSE_PRIOR and a.prediction_source == 1 and b.prediction_source == 0, (k, hex(a.flags), hex(b.flags))
    assert res_chained == plain_chained >= 2


# ---- 6. so_icp_localization_sequence ----------------------------------------------------------------------------------------------------
def _localization_context(factory, sc):
    slam = scene_with_oracle(sc, None, factory, oracle_too=False, max_iterations=spd.MAX_OUTER)[1]
    slam.shift_map(sc.gt_pose(0)[:3])
    return slam


def _map_bytes(slam):
    return slam.export_map_records(stride=12).tobytes()


@pytest.mark.parametrize("kind", spd.U_KINDS)
def test_localization_sequence_equals_the_per_frame_loop_and_its_maps(soicp, gpu_slam_factory, kind):
    sc, scans, pose0, deltas, priors, modes = spd.run_inputs("tiny", kind)
    n = len(scans)
    times = 0.1 * np.arange(1, n + 1)
    seq = _localization_context(gpu_slam_factory, sc)
    seq.set_sequence_priors(priors, modes)
    res = seq.localization_sequence(scans, pose0, deltas, times)
    rc, poses, guesses, stats, n_done = res
    assert rc == 0 and n_done == n, (rc, n_done, seq.last_error())
    # the loop a caller runs today, from the guesses the run reported; the map after every frame
    loop = _localization_context(gpu_slam_factory, sc)
    maps = []
    for k in range(n):
        if k:
            assert np.array_equal(guesses[k], synth.pose_compose(poses[k - 1], deltas[k])), k
        P = spd.frame_prior(priors, modes, k, guesses[k])
        if P is not None:
            loop.set_pose_prior(P)
        lrc, lpose, lst = loop.localization(True, guesses[k], scans[k], times[k])
        assert lrc == 0
        assert lpose.tobytes() == poses[k].tobytes(), (k, modes[k], lpose - poses[k])
        assert_same_bits(lst, stats[k], ("frame", k, "mode", modes[k]))
        assert bool(stats[k].flags & soicp.FLAG_POSE_PRIOR) == (P is not None) and stats[k].prediction_source == lst.prediction_source == (1 if P is not None else 0)
        maps.append(_map_bytes(loop))
    assert _map_bytes(seq) == maps[-1] and seq.map_size() == loop.map_size() > 0
    seq.close(); loop.close()
    # the map after frame m of the run: the run's first m frames are a run of their own (a partial run of the same frames)
    for m in range(1, n):
        part = _localization_context(gpu_slam_factory, sc)
        part.set_sequence_priors(priors[:m], modes[:m])
        pres = part.localization_sequence(scans[:m], pose0, deltas[:m], times[:m])
        assert pres[0] == 0 and pres[4] == m and pres[1].tobytes() == poses[:m].tobytes()
        assert _map_bytes(part) == maps[m - 1], f"the map after frame {m - 1} differs from the per-frame loop's"
        part.close()


# ---- 7. the last frame's normal equations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["small_chunked", "small_sampled"])
def test_last_frame_normal_equations(soicp, gpu_slam_factory, run):
    """test_gpu_pose_prior.py::test_final_normal_equations' comparison and tolerance, on the last frame of a chained run whose prior is
    measured at its guess: JtJ / Jtr minus the host's prior words (T_meas = guesses_out[last]) are the planes' sums at the final pose"""
    sc, scans, pose0, deltas, priors, modes = spd.run_inputs(run, "zero_row")
    assert modes[-1] == spd.AT_GUESS
    slam = _make(gpu_slam_factory, run)
    assert slam.keep_correspondences(True) == 0
    pinned = [slam.host_alloc_like(s) for s in scans]
    slam.set_sequence_priors(priors, modes)
    rc, poses, guesses, stats, n_done = slam.register_sequence(pinned, pose0, deltas)
    assert rc == 0 and n_done == len(scans)
    st = stats[-1]
    assert (st.flags & soicp.FLAG_POSE_PRIOR) and (st.flags & soicp.FLAG_CHAINED), hex(st.flags)
    last = st.iterations[st.n_iterations - 1]
    x = np.array(last.pose_after)
    planes = slam.correspondence_sums(x)[0]
    assert planes.count == last.num_surf_from_scan
    P = spd.frame_prior(priors, modes, len(scans) - 1, guesses[-1])
    s = ppr.host_prior_sums(P, x, last.num_surf_from_scan)
    cost, JtJ, Jtr = s.cost, np.array(s.JtJ[:]), np.array(s.Jtr[:])
    assert np.abs(JtJ).max() > 0
    for got, want in ((np.array(st.JtJ).reshape(6, 6)[IU] - JtJ, np.array(planes.JtJ[:])), (np.array(st.Jtr) - Jtr, np.array(planes.Jtr[:]))):
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), (got, want)
    assert abs((last.final_cost - cost) - planes.cost) <= 1e-9 * max(1.0, abs(planes.cost))
    slam.close()


# ---- 8. state rules ----------------------------------------------------------------------------------------------------------------------
def test_one_shot_count_withdrawal_and_refusals(soicp, gpu_slam_factory):
    sc, scans, pose0, deltas, priors, modes = spd.run_inputs("tiny", "dense")
    scans, deltas, priors, modes = scans[:3], deltas[:3], priors[:3], [spd.GIVEN, spd.AT_GUESS, spd.AT_GUESS]
    priors[0] = spd.frame_prior(priors, [spd.AT_GUESS] * 3, 0, synth.perturb_pose(sc.gt_pose(0), 900, 0.02, 0.2))  # (a finite T_meas for the GIVEN frame)
    slam = _make(gpu_slam_factory, "tiny")
    assert slam.keep_correspondences(True) == 0
    scan, guess = scans[0], pose0
    times = [0.1, 0.2, 0.3]

    def has_prior(res):
        return [bool(st.flags & soicp.FLAG_POSE_PRIOR) for st in res[3]]
    # one-shot: the call after a run with priors carries none
    slam.set_sequence_priors(priors, modes)
    assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [True, True, True]
    assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [False, False, False]
    # NULL modes: all GIVEN
    slam.set_sequence_priors([priors[0]] * 3)
    assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [True, True, True]
    # a call of another length is refused before it touches anything and leaves them pending
    slam.set_sequence_priors(priors, modes)
    for call in (lambda: slam.register_sequence(scans[:2], pose0, deltas[:2]), lambda: slam.localization_sequence(scans[:2], pose0, deltas[:2], times[:2])):
        with pytest.raises(soicp.SoIcpError, match="so_icp error -1: .*count differs"):
            call()
    # ... as do the entries that cannot carry them
    poses2 = np.stack([guess, guess])
    for call in (lambda: slam.register(scan, guess), lambda: slam.register_dev(*slam.upload_scan(scan), guess),
                 lambda: slam.localization(True, guess, scan, 0.1), lambda: slam.localization_dev(True, guess, *slam.upload_scan(scan), 0.1),
                 lambda: slam.register_batch(scan, poses2), lambda: slam.match(scan, guess), lambda: slam.match_dev(*slam.upload_scan(scan), guess),
                 lambda: slam.set_pose_prior(priors[0])):
        with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*priors of a run are pending"):
            call()
    assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [True, True, True], "the refused calls left the priors pending"
    assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [False, False, False]
    # withdrawal: count 0, priors NULL
    for withdraw in (lambda: slam.L.so_icp_set_sequence_priors(slam.h, 0, (soicp.PosePrior * 3)(*priors), None), lambda: slam.set_sequence_priors(None)):
        slam.set_sequence_priors(priors, modes)
        assert withdraw() in (0, None)
        assert slam.register(scan, guess)[0] == 0
        assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [False, False, False]
    # a pending single prior is refused by both sequence entries as before, and by this call; it stays pending
    slam.set_pose_prior(priors[0])
    with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*pose prior is pending"):
        slam.set_sequence_priors(priors, modes)
    with pytest.raises(soicp.SoIcpError, match="so_icp error -5: .*pose prior is pending"):
        slam.register_sequence(scans, pose0, deltas)
    rc, _, st = slam.register(scan, guess)
    assert rc == 0 and (st.flags & soicp.FLAG_POSE_PRIOR)
    # validation: on the words a mode reads
    arr = lambda ps: (soicp.PosePrior * len(ps))(*ps)
    u8 = lambda ms: (C.c_uint8 * len(ms))(*ms)
    set_raw = lambda ps, ms: slam.L.so_icp_set_sequence_priors(slam.h, len(ps), arr(ps), u8(ms) if ms is not None else None)

    def broken(**fields):
        p = soicp.PosePrior.from_buffer_copy(bytes(priors[0]))
        for name, (i, v) in fields.items():
            getattr(p, name)[i] = v
        return p
    assert set_raw([priors[0], broken(sqrt_information=(7, float("nan")))], [spd.GIVEN, spd.GIVEN]) == -1
    assert set_raw([priors[0], broken(count_fraction=(2, float("inf")))], [spd.GIVEN, spd.AT_GUESS]) == -1
    assert set_raw([priors[0], broken(T_meas=(0, float("nan")))], None) == -1
    zero_q = soicp.PosePrior.from_buffer_copy(bytes(priors[0]))
    for i in range(3, 7):
        zero_q.T_meas[i] = 0.0
    assert set_raw([zero_q, priors[0]], [spd.GIVEN, spd.GIVEN]) == -1 and b"zero norm" in slam.L.so_icp_last_error(slam.h)
    assert set_raw([priors[0], priors[0]], [spd.GIVEN, 3]) == -1
    assert has_prior(slam.register_sequence(scans[:2], pose0, deltas[:2])) == [False, False], "a refused call leaves nothing pending"
    # T_meas of an AT_GUESS frame and every word of a NONE frame are not read
    nan_all = soicp.PosePrior.from_buffer_copy(np.full(55, np.nan).tobytes())
    assert set_raw([zero_q, nan_all, broken(T_meas=(0, float("nan")))], [spd.AT_GUESS, spd.NONE, spd.AT_GUESS]) == 0
    assert has_prior(slam.register_sequence(scans, pose0, deltas)) == [True, False, True]
    slam.close()
    # a sharded context
    sharded = gpu_slam_factory(plane_res=sc.plane_res, world_size=2, rank=0)
    assert sharded.L.so_icp_set_sequence_priors(sharded.h, 3, arr(priors), None) == -5
    sharded.close()
    # consumed whatever the call returns: a run that finds too little map
    empty = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=spd.MAX_OUTER)
    empty.set_sequence_priors(priors, modes)
    assert empty.register_sequence(scans, pose0, deltas)[0] == 1  # SO_ICP_NOT_ENOUGH_MAP_FEATURES
    assert empty.register(scan, guess)[0] == 1, "the priors were consumed: so_icp_register is not refused"
    empty.close()


# ---- 9. the adapter -----------------------------------------------------------------------------------------------------------------------
def _between(a, b):
    """adapter_driver.cpp between(): a^-1 * b, operation by operation in IEEE double"""
    a = [float(v) for v in a]; b = [float(v) for v in b]
    ax, ay, az, aw = -a[3], -a[4], -a[5], a[6]
    vx, vy, vz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    cx = ay * vz - az * vy; cy = az * vx - ax * vz; cz = ax * vy - ay * vx
    tx = vx + 2 * (aw * cx + ay * cz - az * cy); ty = vy + 2 * (aw * cy + az * cx - ax * cz); tz = vz + 2 * (aw * cz + ax * cy - ay * cx)
    rx, ry, rz, rw = b[3], b[4], b[5], b[6]
    w = aw * rw - ax * rx - ay * ry - az * rz
    x = aw * rx + ax * rw + ay * rz - az * ry
    y = aw * ry - ax * rz + ay * rw + az * rx
    z = aw * rz + ax * ry - ay * rx + az * rw
    return np.array([tx, ty, tz, x, y, z, w])


def test_adapter_driver_sequence_prior_at_guess(soicp, gpu_slam_factory, tmp_path):
    assert os.path.exists(DRIVER), "adapter/adapter_driver not built: run python __graft_entry__.py"
    sc = synth.Scene("tiny")
    n_frames, max_it = 6, 4
    scans = [np.ascontiguousarray(sc.scan(i), np.float32) for i in range(n_frames)]
    guesses = [sc.gt_pose(0)] + [sc.guess(i) for i in range(1, n_frames)]
    times = [0.1 * i for i in range(n_frames)]
    fin = tmp_path / "in.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ifii", n_frames, sc.plane_res, max_it, -1))
        for i in range(n_frames):
            f.write(struct.pack("<i", len(scans[i])))
            f.write(np.asarray(guesses[i], np.float64).tobytes()); f.write(struct.pack("<d", times[i])); f.write(scans[i].tobytes())
    outs = {}
    for flags in ((), ("--prior-at-guess",)):
        fout = tmp_path / f"out{len(flags)}.bin"
        r = subprocess.run([DRIVER, str(fin), str(fout), "--sequence", *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = open(fout, "rb").read()
        status, n_done = struct.unpack_from("<ii", raw, 0)
        assert status == 0 and n_done == n_frames - 1, (flags, status, n_done)
        outs[flags] = raw
    assert outs[()] != outs[("--prior-at-guess",)], "the priors changed nothing"
    # the same run through ctypes: the driver's U (that of --vio-prior, the uncertainty terms at 0) at the guess of every frame
    deltas = np.zeros((n_frames - 1, 7)); deltas[:, 6] = 1.0
    for k in range(1, n_frames - 1):
        deltas[k] = _between(guesses[k], guesses[k + 1])
    prior = ppr.reference_prior([0, 0, 0, 0, 0, 0, 1.0], [0.0, 0.0, 0.0], 0.9)
    for flags, raw in outs.items():
        slam = gpu_slam_factory(plane_res=sc.plane_res, line_res=sc.plane_res / 2, max_surface_features=-1, max_iterations=max_it)
        assert slam.localization(False, guesses[0], scans[0], times[0])[0] == 2
        if flags:
            slam.set_sequence_priors([prior] * (n_frames - 1), [spd.AT_GUESS] * (n_frames - 1))
        res = slam.localization_sequence(scans[1:], guesses[1], deltas, times[1:])
        assert res[0] == 0 and res[4] == n_frames - 1
        assert all(bool(st.flags & soicp.FLAG_POSE_PRIOR) == bool(flags) for st in res[3])
        assert raw[8:] == np.ascontiguousarray(res[1], np.float64).tobytes(), (flags, np.frombuffer(raw, np.float64, 7 * (n_frames - 1), 8).reshape(-1, 7) - res[1])
        slam.close()
