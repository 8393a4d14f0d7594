"""CPU: tests/correspondences_ref.py -- the plain-numpy statement of what so_icp_correspondences exports -- held to the oracle
(orc_register's last correspondences, orc_evaluate), and the binding's two structs held to the header.  The GPU tests
(test_gpu_correspondences.py) then hold the device to that restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import correspondences_ref as cref
from superodom_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (scene, points of scan 0 taken, max_surface_features)
CASES = [("tiny", 4096, -1), ("tiny", 4096, 2000), ("tiny", 2049, -1), ("tiny", 65, -1), ("tiny", 1, -1), ("small", 16384, -1), ("small", 1, -1)]
_cache = {}


def _registered(oracle, scene, n, msf, variant=0, composite=False):
    """(scene, scan, corrs of the last outer iteration, oracle Stats) of scan 0's first n points, registered once per session"""
    key = (scene, n, msf, variant, composite)
    if key not in _cache:
        sc = synth.Scene(scene)
        om = oracle.OracleMap(plane_res=sc.plane_res)
        om.add_surf(sc.map_points)
        scan = np.ascontiguousarray(sc.scan(0)[:n], np.float32)
        if composite:
            scan, _ = cref.composite_scan(scan, 1024)
        rc, pose, st, corrs = om.register(scan, sc.guess(0), oracle.default_config(max_iterations=5, max_surface_features=msf, tukey_variant=variant),
                                          want_corrs=True)
        assert rc == 0 and st.n_iterations >= 1
        _cache[key] = (sc, scan, corrs, st)
    return _cache[key]


def _within(got, want, n_terms, abs_sum, what):
    got, want, bound = np.asarray(got, float), np.asarray(want, float), cref.sum_bound(n_terms, np.asarray(abs_sum, float))
    err = np.abs(got - want)
    print(f"{what}: max |difference| {err.max():.3e}, largest |difference| / bound {np.max(err[bound > 0] / bound[bound > 0], initial=0.0):.3f}")
    assert np.all(err <= bound), (what, float(err.max()), float(np.min(bound)))


@pytest.mark.parametrize("scene,n,msf", CASES)
def test_restatement_reproduces_the_oracle_at_the_default_pose(oracle, scene, n, msf):
    sc, scan, corrs, st = _registered(oracle, scene, n, msf)
    last = st.iters[st.n_iterations - 1]
    pose = np.array(last.pose_after)
    e = cref.expected(corrs, pose, sc.plane_res, 0)
    N = len(e["records"])
    assert N == last.num_surf and N == int((corrs["status"] == 0).sum())
    # the records: ascending positions of status 0, the scan's own bits, 254 for the points the sampling rule dropped
    assert np.array_equal(e["records"]["index"], np.flatnonzero(corrs["status"] == 0)) and np.all(np.diff(e["records"]["index"].astype(np.int64)) > 0)
    assert np.array_equal(e["records"]["p"], scan[e["records"]["index"]])
    assert np.array_equal(e["status"] == cref.NOT_SAMPLED, corrs["status"] < 0)
    assert (msf > 0 and n > msf) == bool((e["status"] == cref.NOT_SAMPLED).any())
    assert np.array_equal(np.isnan(e["residual"]), corrs["status"] != 0)
    # orc_evaluate on the same correspondences and pose, and what orc_register itself reported there
    cost, JtJ, Jtr, cnt = oracle.evaluate(corrs, pose, sc.plane_res, 0)
    assert cnt == N
    for tag, (c0, J0, r0) in {"orc_evaluate": (cost, JtJ, Jtr), "orc_register": (last.final_cost, np.array(st.JtJ).reshape(6, 6), np.array(st.Jtr))}.items():
        _within(e["cost"], c0, N, e["cost_abs"], f"{tag} cost")
        _within(e["JtJ"], J0, N, e["JtJ_abs"], f"{tag} JtJ")
        _within(e["Jtr"], r0, N, e["Jtr_abs"], f"{tag} Jtr")
    # at the default pose no correspondence of these scans lies outside Tukey's window
    if N:
        assert np.abs(e["records"]["residual"]).max() ** 2 < e["a2"]


@pytest.mark.parametrize("variant", [0, 1])
def test_restatement_reproduces_orc_evaluate_on_both_tukey_branches(oracle, variant):
    """the composite scan (runs of far points, which the oracle gives status 1) evaluated 1 m above the optimised pose: part of the
    set is outside the loss's window, part inside"""
    sc, scan, corrs, st = _registered(oracle, "tiny", 4096, -1, variant, composite=True)
    _, far = cref.composite_scan(np.ascontiguousarray(sc.scan(0), np.float32), 1024)
    assert np.all(corrs["status"][far] == 1)
    pose = np.array(st.iters[st.n_iterations - 1].pose_after); pose[2] += 1.0
    e = cref.expected(corrs, pose, sc.plane_res, variant)
    outside = e["records"]["residual"] ** 2 > e["a2"]
    assert outside.any() and (~outside).any(), "both branches of the loss must run"
    assert np.all(e["records"]["weight"][outside] == 0) and np.all(e["records"]["weight"][~outside] >= 0)
    cost, JtJ, Jtr, cnt = oracle.evaluate(corrs, pose, sc.plane_res, variant)
    N = len(e["records"])
    assert cnt == N
    _within(e["cost"], cost, N, e["cost_abs"], "cost"); _within(e["JtJ"], JtJ, N, e["JtJ_abs"], "JtJ"); _within(e["Jtr"], Jtr, N, e["Jtr_abs"], "Jtr")


def test_far_points_do_not_change_the_registration(oracle):
    """a point at x >= 5 000 m lies outside the window: status 1, and the pose is that of the run without such points, bit for bit"""
    sc, scan, corrs, st = _registered(oracle, "tiny", 4096, -1, 0, composite=True)
    _, far = cref.composite_scan(np.ascontiguousarray(sc.scan(0), np.float32), 1024)
    om = oracle.OracleMap(plane_res=sc.plane_res)
    om.add_surf(sc.map_points)
    rc, pose, st2, _ = om.register(scan[~far], sc.guess(0), oracle.default_config(max_iterations=5))
    assert rc == 0 and st2.n_iterations == st.n_iterations
    assert bytes(st2.iters[st2.n_iterations - 1].pose_after) == bytes(st.iters[st.n_iterations - 1].pose_after)


def test_correspondence_structs_match_the_header(soicp, tmp_path):
    fields = {"so_icp_correspondence": (soicp.Correspondence, ["index", "p", "n", "d", "coeff", "residual", "weight"]),
              "so_icp_correspondence_info": (soicp.CorrespondenceInfo, ["n_points", "n_accepted", "valid", "outer_iteration", "pose_fit", "pose_eval", "cost"])}
    items, want = [], []
    for name, (cls, fs) in fields.items():
        items.append(f"sizeof({name})"); want.append(C.sizeof(cls))
        for f in fs:
            items.append(f"offsetof({name}, {f})"); want.append(getattr(cls, f).offset)
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "so_icp.h"\nint main(){size_t v[] = {' + ", ".join(items) +
                   '};for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu\\n", v[i]);return 0;}')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)]).split())) == want
    assert C.sizeof(soicp.Correspondence) == 72 == soicp.CORRESPONDENCE_DTYPE.itemsize == cref.RECORD_DTYPE.itemsize
    assert [(n, soicp.CORRESPONDENCE_DTYPE.fields[n][1]) for n in soicp.CORRESPONDENCE_DTYPE.names] == \
           [(f, getattr(soicp.Correspondence, f).offset) for f in fields["so_icp_correspondence"][1]]
    L = soicp.load()
    for sym in ("so_icp_keep_correspondences", "so_icp_correspondences"):
        assert sym in soicp.EXPORTED and getattr(L, sym)
    assert L.so_icp_abi_version() == 4


def test_host_only_context_refuses_the_correspondence_entries(soicp):
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    assert host.keep_correspondences(True) == -2  # SO_ICP_E_HIP
    with pytest.raises(soicp.SoIcpError, match="no CPU fallback"):
        host.correspondences(cap=16)
