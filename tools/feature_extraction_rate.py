"""Rates of so_icp_extract_features on the GPU box (results in profiles/feature_extraction/), for the 131 072-point Ouster sweep
(os1_128-like, 1024 x 128) and the 28 800-point VLP-16 sweep, each de-skewed against an IMU buffer, filter_point_size 3:
  * host payload in, both clouds out (so_icp_extract_features)
  * payload resident in HBM, clouds left there (so_icp_extract_features_dev)
  * the resident chain sweep -> features -> so_icp_prefilter_scan_dev -> so_icp_localization_dev against the same chain through
    host buffers (so_icp_extract_features -> so_icp_prefilter_scan -> so_icp_localization), ms per frame
  * the CPU restatement (numpy ingest and sampling + the C oracle's de-skew, one core), labelled as such
    python tools/feature_extraction_rate.py [--reps N] [--kernels-only] [--livox | --registered-scan [--only ouster|livox]]
--kernels-only: only the resident entry, for a rocprofv3 --kernel-trace --stats run.
--livox: the same rows for so_icp_extract_features_livox instead (results in profiles/feature_extraction/rate_livox.txt): seeded
Mid-360-like sweeps (synth.livox_sweep) of 20 000 and of 131 072 CustomPoints, R = a few degrees of roll and pitch, the chain at
the livox_mid360 operating point (planeRes 0.1, 4 000 surface features).
--registered-scan: the step behind the chain, laserMapping::publishTopic's registered scan of the full-resolution de-skewed sweep
(results in profiles/feature_extraction/rate_registered_scan.txt), for the 131 072-point Ouster sweep and a 20 000-point Mid-360-like
sweep (whose rejected points are zero records, dropped here).  Rows, alternated inside every round, best of 3 rounds of --reps calls
and the rounds' spread:
  * so_icp_transform_cloud in a pinned buffer + the squeeze on the host (what the node shell did before; numpy's mask compaction
    stands in for its record-by-record loop)
  * so_icp_registered_scan in that pinned buffer, out == records
  * so_icp_registered_scan_dev on *d_nodistortion_out, with the copy to a pinned host buffer and without
  * the chain sweep -> features -> pre-filter -> localization -> registered scan, resident against host entries, ms per frame"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import deskew_data as dd  # noqa: E402
import feature_extraction_ref as fr  # noqa: E402
import livox_ref as lr  # noqa: E402
from superodom_amd import binding, synth  # noqa: E402

T0 = 1.7e9 + 0.25


def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def _best_ms(fn, reps, rounds=3):
    fn()
    best = float("inf")
    for _ in range(rounds):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        best = min(best, 1e3 * (time.perf_counter() - t) / reps)
    return best


def rates(name, buf, w, h, rs, sensor, reps, kernels_only):
    hip = _hip()
    layout = fr.layout_for(sensor, 3, 0.2, row_step=rs)
    poses = dd.pose_buffer(T0, seed=22, translate=False)
    pp = np.ascontiguousarray(poses)
    ppp = pp.ctypes.data_as(C.POINTER(C.c_double))
    n = w * h
    slam = binding.LidarSlamGpu(plane_res=0.2, max_iterations=4)
    L = slam.L
    info = binding.FeatureInfo()
    d_raw = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_raw), buf.nbytes) == 0
    assert hip.hipMemcpy(d_raw, buf.ctypes.data_as(C.c_void_p), buf.nbytes, 1) == 0
    d_rec, d_surf = C.c_void_p(), C.c_void_p()

    def dev():
        rc = L.so_icp_extract_features_dev(slam.h, d_raw, w, h, C.byref(layout), T0, ppp, len(pp), 1, None, C.byref(d_rec), C.byref(d_surf),
                                           C.byref(info))
        assert rc == 0, rc
    if kernels_only:
        for _ in range(reps):
            dev()
        hip.hipFree(d_raw)
        return
    rec_out = np.empty((n, 32), np.uint8)
    surf_out = np.empty((n, 32), np.uint8)

    def host():
        rc = L.so_icp_extract_features(slam.h, buf.ctypes.data_as(C.c_void_p), w, h, C.byref(layout), T0, ppp, len(pp), 1, None,
                                       rec_out.ctypes.data_as(C.c_void_p), surf_out.ctypes.data_as(C.c_void_p), C.byref(info))
        assert rc == 0, rc
    host_ms = _best_ms(host, reps)
    dev_ms = _best_ms(dev, reps)
    n_surf = info.n_surface

    # chains: a map seeded with the first frame, then every call registers (and inserts) the same sweep again
    chain = {}
    for mode in ("host", "dev"):
        s = binding.LidarSlamGpu(plane_res=0.2, max_iterations=4)
        pose = np.array([0, 0, 0, 0, 0, 0, 1.0])
        k = [0]

        def step(first=False):
            t = T0 + 0.1 * k[0]
            k[0] += 1
            if mode == "dev":
                _, ds, inf = s.extract_features_dev(d_raw.value, w, h, layout, T0, poses, True, None)
                dp, nf, _ = s.prefilter_scan_dev(ds, inf.n_surface, 32, 1, 0.2, 0.4)
                rc, _, _ = s.localization_dev(0 if first else 1, pose, dp, nf, t)
            else:
                _, sf, _ = s.extract_features(buf, w, h, layout, T0, poses, True, None)
                dp, nf, _ = s.prefilter_scan(sf.view(np.float32)[:, :3], 1, 0.2, 0.4)
                rc, _, _ = s.localization(0 if first else 1, pose, s.download_scan(dp, nf), t)
            assert rc in (0, 2), rc
        step(first=True)
        chain[mode] = _best_ms(step, max(reps // 5, 5))
        s.close()
    hip.hipFree(d_raw)

    t = time.perf_counter()
    import oracle_py
    rec = fr.ingest(buf, w, h, layout)
    rec, _, _ = oracle_py.deskew(rec, 20, T0, poses, True, None)
    fr.surf_sample(rec, 3, 0.2)
    cpu_ms = 1e3 * (time.perf_counter() - t)
    print(f"{name}: {n} points, {len(poses)} IMU poses, filter_point_size 3 -> {n_surf} surf points")
    print(f"  host payload in, both clouds out  {host_ms:.3f} ms")
    print(f"  resident in HBM                   {dev_ms:.3f} ms  (pose table upload + 2 kernels + count read-back)")
    print(f"  chain features -> prefilter -> localization: resident {chain['dev']:.3f} ms, through host buffers {chain['host']:.3f} ms per frame")
    print(f"  CPU restatement (numpy ingest + sampling, C oracle de-skew; one core, not the reference's code) {cpu_ms:.1f} ms")


def rates_livox(n, reps, kernels_only):
    hip = _hip()
    vals = synth.livox_sweep(n=n, seed=1)
    buf = synth.livox_points(vals)
    layout = binding.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
    poses = dd.pose_buffer(T0, seed=22, translate=False)
    slam = binding.LidarSlamGpu(plane_res=0.1, line_res=0.05, max_surface_features=4000, max_iterations=4)
    d_raw = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_raw), buf.nbytes) == 0
    assert hip.hipMemcpy(d_raw, buf.ctypes.data_as(C.c_void_p), buf.nbytes, 1) == 0
    info = [None]

    def dev():
        info[0] = slam.extract_features_livox_dev(d_raw.value, n, layout, T0, poses, True, None)[2]
    if kernels_only:
        for _ in range(reps):
            dev()
        hip.hipFree(d_raw)
        return

    def host():
        slam.extract_features_livox(buf, n, layout, T0, poses, True, None)
    host_ms = _best_ms(host, reps)
    dev_ms = _best_ms(dev, reps)

    # chains: a map seeded with the first frame, then every call registers (and inserts) the same sweep again
    chain = {}
    for mode in ("host", "dev"):
        s = binding.LidarSlamGpu(plane_res=0.1, line_res=0.05, max_surface_features=4000, max_iterations=4)
        pose = np.array([0, 0, 0, 0, 0, 0, 1.0])
        k = [0]

        def step(first=False):
            t = T0 + 0.1 * k[0]
            k[0] += 1
            if mode == "dev":
                _, ds, inf = s.extract_features_livox_dev(d_raw.value, n, layout, T0, poses, True, None)
                dp, nf, _ = s.prefilter_scan_dev(ds, inf.n_surface, 32, 1, 0.05, 0.1)
                rc, _, _ = s.localization_dev(0 if first else 1, pose, dp, nf, t)
            else:
                _, sf, _ = s.extract_features_livox(buf, n, layout, T0, poses, True, None)
                dp, nf, _ = s.prefilter_scan(sf.view(np.float32)[:, :3], 1, 0.05, 0.1)
                rc, _, _ = s.localization(0 if first else 1, pose, s.download_scan(dp, nf), t)
            assert rc in (0, 2), rc
        step(first=True)
        chain[mode] = _best_ms(step, max(reps // 5, 5))
        s.close()
    hip.hipFree(d_raw)

    t = time.perf_counter()
    import oracle_py
    rec = lr.ingest(vals, lr.R_TILT)
    rec, _, _ = oracle_py.deskew(rec, 20, T0, poses, True, None)
    fr.surf_sample(rec, 3, 0.2)
    cpu_ms = 1e3 * (time.perf_counter() - t)
    print(f"Livox CustomMsg, Mid-360-like: {n} points ({buf.nbytes} bytes), {len(poses)} IMU poses, filter_point_size 3 -> {info[0].n_surface} surf points")
    print(f"  host payload in, both clouds out  {host_ms:.3f} ms")
    print(f"  resident in HBM                   {dev_ms:.3f} ms  (pose table upload + 2 kernels + count read-back)")
    print(f"  chain features -> prefilter -> localization (planeRes 0.1, 4000 features): resident {chain['dev']:.3f} ms, through host buffers {chain['host']:.3f} ms per frame")
    print(f"  CPU restatement (numpy ingest + sampling, C oracle de-skew; one core, not the reference's code) {cpu_ms:.1f} ms")


def _rounds_ms(rows, reps, rounds=3):
    """rows: {name: fn}; every round times each row in turn (alternated); returns {name: [ms per call of each round]}"""
    for fn in rows.values():
        fn()
    out = {k: [] for k in rows}
    for _ in range(rounds):
        for k, fn in rows.items():
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            out[k].append(1e3 * (time.perf_counter() - t) / reps)
    return out


def rates_registered_scan(name, reps, kernels_only):
    """name: "ouster" (131 072 points) or "livox" (20 000 points)"""
    hip = _hip()
    poses = dd.pose_buffer(T0, seed=22, translate=False)
    T = np.concatenate([[3.0, -4.0, 0.5], synth.quat_from_rotvec(np.array([0.02, -0.03, 0.8]))])
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    if name == "ouster":
        buf, w, h, rs, _ = fr.ouster_sweep(1024, 128, seed=1, nan_every=997, zero_every=61)
        n = w * h
        layout = fr.layout_for(fr.SENSOR_OUSTER, 3, 0.2, row_step=rs)
        cfg = dict(plane_res=0.2, max_iterations=4)
        res = (0.2, 0.4)
        title = f"os1_128-like Ouster: {n} points"
    else:
        n = 20000
        buf = synth.livox_points(synth.livox_sweep(n=n, seed=1))
        layout = binding.livox_layout(3, 0.2, R_imu_laser_gravity=lr.R_TILT)
        cfg = dict(plane_res=0.1, line_res=0.05, max_surface_features=4000, max_iterations=4)
        res = (0.05, 0.1)
        title = f"Livox CustomMsg, Mid-360-like: {n} points"
    d_raw = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_raw), buf.nbytes) == 0
    assert hip.hipMemcpy(d_raw, buf.ctypes.data_as(C.c_void_p), buf.nbytes, 1) == 0

    def features_dev(s):
        if name == "ouster":
            return s.extract_features_dev(d_raw.value, w, h, layout, T0, poses, True, None)
        return s.extract_features_livox_dev(d_raw.value, n, layout, T0, poses, True, None)

    def features_host(s):
        if name == "ouster":
            return s.extract_features(buf, w, h, layout, T0, poses, True, None)
        return s.extract_features_livox(buf, n, layout, T0, poses, True, None)

    slam = binding.LidarSlamGpu(**cfg)
    L = slam.L
    d_rec, _, _ = features_dev(slam)
    nk = C.c_size_t(0)
    d_out = C.c_void_p()

    def dev_resident():
        rc = L.so_icp_registered_scan_dev(slam.h, d_rec, n, 32, Tp, None, C.byref(d_out), C.byref(nk))
        assert rc == 0, rc
    if kernels_only:
        for _ in range(reps):
            dev_resident()
        hip.hipFree(d_raw)
        return
    rec = np.empty((n, 32), np.uint8)
    assert hip.hipMemcpy(rec.ctypes.data_as(C.c_void_p), d_rec, rec.nbytes, 2) == 0
    work = slam.host_alloc_like(rec)   # the node shell's pinned message buffer
    out_pinned = slam.host_alloc_like(rec)
    keep = np.zeros(n, np.uint8)
    kept = {}

    def old():
        work[...] = rec
        rc = L.so_icp_transform_cloud(slam.h, work.ctypes.data_as(C.c_void_p), n, 32, Tp, keep.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nk))
        assert rc == 0, rc
        if nk.value != n:
            m = work[keep.view(bool)]
            work[:len(m)] = m
        kept["old"] = nk.value

    def new_host():
        work[...] = rec
        rc = L.so_icp_registered_scan(slam.h, work.ctypes.data_as(C.c_void_p), n, 32, Tp, work.ctypes.data_as(C.c_void_p), C.byref(nk))
        assert rc == 0, rc
        kept["new"] = nk.value

    def dev_with_copy():
        rc = L.so_icp_registered_scan_dev(slam.h, d_rec, n, 32, Tp, out_pinned.ctypes.data_as(C.c_void_p), C.byref(d_out), C.byref(nk))
        assert rc == 0, rc
    rows = _rounds_ms({"old": old, "new_host": new_host, "dev_copy": dev_with_copy, "dev": dev_resident}, reps)
    old(); a = work[:kept["old"]].copy()
    new_host(); b = work[:kept["new"]].copy()
    dev_with_copy()
    assert kept["old"] == kept["new"] == nk.value and np.array_equal(a, b) and np.array_equal(b, out_pinned[:nk.value]), "the rows publish the same bytes"

    # chains: a map seeded with the first frame, then every call registers (and inserts) the same sweep again and builds its registered scan
    chain = {}
    steps = {}
    ctxs = []
    for mode in ("host", "dev"):
        s = binding.LidarSlamGpu(**cfg)
        ctxs.append(s)
        pose = np.array([0, 0, 0, 0, 0, 0, 1.0])
        k = [0]

        def step(first=False, s=s, mode=mode, k=k, pose=pose):
            t = T0 + 0.1 * k[0]
            k[0] += 1
            if mode == "dev":
                dr, ds, inf = features_dev(s)
                dp, nf, _ = s.prefilter_scan_dev(ds, inf.n_surface, 32, 1, *res)
                rc, p, _ = s.localization_dev(0 if first else 1, pose, dp, nf, t)
                s.registered_scan_dev(dr, n, 32, p)
            else:
                nd, sf, _ = features_host(s)
                dp, nf, _ = s.prefilter_scan(sf.view(np.float32)[:, :3], 1, *res)
                rc, p, _ = s.localization(0 if first else 1, pose, s.download_scan(dp, nf), t)
                s.registered_scan(nd, p)
            assert rc in (0, 2), rc
        step(first=True)
        steps[mode] = step
    chain = _rounds_ms(steps, max(reps // 5, 5))
    for s in ctxs:
        s.close()
    hip.hipFree(d_raw)

    def fmt(v):
        return f"{min(v):.3f} ms  (rounds {', '.join(f'{x:.3f}' for x in v)})"
    print(f"{title}, {kept['old']} kept by the registered scan ({n - kept['old']} dropped), records of 32 bytes")
    print(f"  so_icp_transform_cloud in a pinned buffer + host squeeze   {fmt(rows['old'])}")
    print(f"  so_icp_registered_scan, out == records (pinned)            {fmt(rows['new_host'])}")
    print(f"  so_icp_registered_scan_dev on *d_nodistortion_out + copy   {fmt(rows['dev_copy'])}")
    print(f"  so_icp_registered_scan_dev, result left in HBM             {fmt(rows['dev'])}")
    print(f"  chain features -> prefilter -> localization -> registered scan: resident {fmt(chain['dev'])}")
    print(f"                                                      through host buffers {fmt(chain['host'])}")


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
    ko = "--kernels-only" in sys.argv
    if "--registered-scan" in sys.argv:
        only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
        for name in ("ouster", "livox"):
            if only in (None, name):
                rates_registered_scan(name, reps, ko)
        return
    if "--livox" in sys.argv:
        for n in (20000, 131072):
            rates_livox(n, reps, ko)
        return
    buf, w, h, rs, _ = fr.ouster_sweep(1024, 128, seed=1, nan_every=997, zero_every=61)
    rates("os1_128-like Ouster", buf, w, h, rs, fr.SENSOR_OUSTER, reps, ko)
    buf, w, h, rs, _ = fr.velodyne_sweep(28800, seed=1, nan_every=499, zero_every=73)
    rates("VLP-16", buf, w, h, rs, fr.SENSOR_VELODYNE, reps, ko)


if __name__ == "__main__":
    main()
