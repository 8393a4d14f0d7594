"""CPU-side checks of so_icp_localization_sequence (register + insert per frame over a run): the symbol is exported, invalid
arguments are refused with SO_ICP_E_INVALID, a host-only context (device_id < 0) fails with SO_ICP_E_HIP without touching its map,
and an empty run does nothing.  No compute kernels run here."""
import ctypes as C

import numpy as np

from helpers import noisy_planes_cloud

E_INVALID, E_HIP = -1, -2


def _args(n_frames, scans=None):
    count = n_frames
    ptrs = (C.c_void_p * max(count, 1))(); ns = (C.c_size_t * max(count, 1))()
    for k, sc in enumerate(scans or []):
        ptrs[k], ns[k] = sc.ctypes.data, len(sc)
    pose0 = np.array([0, 0, 0, 0, 0, 0, 1.0]); deltas = np.zeros((max(count, 1), 7)); deltas[:, 6] = 1.0
    times = np.arange(max(count, 1), dtype=np.float64) * 0.1
    out = np.zeros((max(count, 1), 7)); guesses = np.zeros((max(count, 1), 7))
    return ptrs, ns, pose0, deltas, times, out, guesses


def _f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_symbol_is_exported(soicp):
    L = soicp.load()
    assert hasattr(L, "so_icp_localization_sequence")
    assert "so_icp_localization_sequence" in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4


def test_invalid_arguments(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    scans = [np.zeros((10, 3), np.float32) for _ in range(3)]
    ptrs, ns, pose0, deltas, times, out, guesses = _args(3, scans)
    n_done = C.c_int32(7)
    f = L.so_icp_localization_sequence
    # no context
    assert f(None, 3, ptrs, ns, 12, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), _f64(guesses), None, C.byref(n_done)) == E_INVALID
    assert n_done.value == 0
    # negative count
    assert f(host.h, -1, ptrs, ns, 12, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), _f64(guesses), None, None) == E_INVALID
    # missing arrays: scans, n_points, pose0, times, poses_out; deltas with more than one frame
    assert f(host.h, 3, None, ns, 12, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), None, None, None) == E_INVALID
    assert f(host.h, 3, ptrs, None, 12, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), None, None, None) == E_INVALID
    assert f(host.h, 3, ptrs, ns, 12, 0, None, _f64(deltas), _f64(times), _f64(out), None, None, None) == E_INVALID
    assert f(host.h, 3, ptrs, ns, 12, 0, _f64(pose0), _f64(deltas), None, _f64(out), None, None, None) == E_INVALID
    assert f(host.h, 3, ptrs, ns, 12, 0, _f64(pose0), _f64(deltas), _f64(times), None, None, None, None) == E_INVALID
    assert f(host.h, 3, ptrs, ns, 12, 0, _f64(pose0), None, _f64(times), _f64(out), None, None, None) == E_INVALID
    # a NULL scan with points, a stride that is not a multiple of 4, a strided resident scan
    bad = (C.c_void_p * 3)(ptrs[0], None, ptrs[2])
    assert f(host.h, 3, bad, ns, 12, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), None, None, None) == E_INVALID
    assert "scans[1]" in host.last_error()
    assert f(host.h, 3, ptrs, ns, 14, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), None, None, None) == E_INVALID
    assert f(host.h, 3, ptrs, ns, 32, 1, _f64(pose0), _f64(deltas), _f64(times), _f64(out), None, None, None) == E_INVALID
    host.close()


def test_host_only_context_fails_without_touching_its_map(soicp):
    L = soicp.load()
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    host.add_surf_point_cloud(noisy_planes_cloud(2000, np.random.default_rng(3)))
    before_n, before = host.map_size(), host.export_map()
    scans = [np.ascontiguousarray(noisy_planes_cloud(500, np.random.default_rng(10 + k)), dtype=np.float32) for k in range(3)]
    ptrs, ns, pose0, deltas, times, out, guesses = _args(3, scans)
    n_done = C.c_int32(5)
    rc = L.so_icp_localization_sequence(host.h, 3, ptrs, ns, 12, 0, _f64(pose0), _f64(deltas), _f64(times), _f64(out), _f64(guesses),
                                        None, C.byref(n_done))
    assert rc == E_HIP and n_done.value == 0
    assert "no CPU fallback" in host.last_error()
    assert host.map_size() == before_n
    assert np.array_equal(host.export_map(), before)
    assert not out.any()
    host.close()


def test_an_empty_run_is_a_no_op(soicp):
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    host.add_surf_point_cloud(noisy_planes_cloud(1000, np.random.default_rng(4)))
    before = host.export_map()
    rc, poses, guesses, stats, n_done = host.localization_sequence([], np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros((0, 7)), np.zeros(0))
    assert rc == 0 and n_done == 0 and poses.shape == (0, 7) and stats == []
    assert np.array_equal(host.export_map(), before)
    host.close()
